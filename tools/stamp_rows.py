"""Where a -DTOLG_STAMPS build leaves its cycle stamps: the ST_* constants of csrc/tolg_stamps.h (rows of alpha_hist /
mu_hist, the workgroup that reports), read from the source so that the kernels and the tools cannot disagree.
`python tools/stamp_rows.py` prints them."""
import os
import re

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trajectory_optimization_matrix_lie_groups_amd", "csrc",
                    "tolg_stamps.h")
ST = {k: int(v) for k, v in re.findall(r"\bST_([A-Z0-9_]+) = (\d+)", open(_SRC).read())}
ROLL, HELPER, POSE, K2, K2_CLOCK = (ST[k] for k in ("ROW_ROLL", "ROW_HELPER", "ROW_POSE", "ROW_K2", "ROW_K2_CLOCK"))
MIN_BATCH = max(ROLL, HELPER + 1, POSE, K2, K2_CLOCK) + 1   # stamps_flush refuses a batch without these rows
MIN_ITERATIONS = 8                                         # ... or a history row shorter than the phases


def row(hist, r, n):
    """Phases 0 .. n-1 of row r of a history tensor [B, max_iter]; a batch or a history the flush refused is an error here."""
    if hist.shape[0] <= r or hist.shape[1] < n:
        raise SystemExit("stamps need a batch of at least %d and %d iterations: history is %s" % (MIN_BATCH, MIN_ITERATIONS, tuple(hist.shape)))
    return hist[r, :n].cpu().numpy()


if __name__ == "__main__":
    for k, v in sorted(ST.items()):
        print("ST_%s = %d" % (k, v))

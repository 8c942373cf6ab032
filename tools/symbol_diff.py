"""Compare the device code of two builds of the library symbol by symbol:
    python tools/symbol_diff.py [--rename PATTERN REPLACEMENT ...] A.so B.so [substring ...]

Per symbol one of
  identical          the same instructions with the same operands in the same order (addresses stripped)
  same instructions  the same sorted list of instructions once register numbers are masked: register assignment and the order
                     of independent instructions moved, the operations did not
  different          anything else (a symbol only one side has included)
then the three counts.  Exit status 1 if a symbol is different.  With substrings: only the symbols whose demangled name
holds one of them.

Symbols pair by name, so one that B.so spells otherwise shows as two different ones.  --rename (any number of them, applied
in order) rewrites the demangled names of A.so with re.sub before the pairing:
    --rename 'k_policy_rollout_lim<(\\d+, \\d+, \\d+, \\d+)' 'k_policy_rollout<\\1, tolg::PolicyLim'
pairs k_policy_rollout_lim<4, 0, 0, 0> of A.so with k_policy_rollout<4, 0, 0, 0, tolg::PolicyLim> of B.so."""
import os
import re
import subprocess
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import _dpp_lint  # noqa: E402

_REGNO = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def _mask(m):
    """v17 -> v, s[4:7] -> s[4]: the register file and the width stay, the numbers go."""
    r = m.group(2)
    if r[0] != "[":
        return m.group(1)
    lo, hi = r[1:-1].split(":")
    return "%s[%d]" % (m.group(1), int(hi) - int(lo) + 1)


def symbols(lib):
    """{symbol: [instruction text, address comment and branch-target address stripped]}"""
    out, cur = {}, None
    for ln in _dpp_lint.disassemble(lib).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:", ln)
        if m and cur is not None:
            cur.append(re.sub(r"\s+", " ", re.sub(r"\s*<[^>]*>$", "", m.group(1))))
    return out


def by_name(syms):
    """{mangled symbol: instructions} -> {demangled name: instructions}.  The name stops ahead of the argument list where that
    still tells the symbols of the library apart, and keeps it where two of them share the rest."""
    full = subprocess.check_output(["c++filt"], input="\n".join(syms).encode()).decode().splitlines() if syms else []
    short = [f.split("(")[0] for f in full]
    shared = {n for n, k in Counter(short).items() if k > 1}
    return {(f if s in shared else s): syms[sym] for sym, f, s in zip(syms, full, short)}


def classify(a, b):
    if a == b:
        return "identical"
    if a is None or b is None or len(a) != len(b):
        return "different"
    # a lone integer operand is a distance in instructions (a jump's): it moves with the order of the instructions between, so
    # it is masked with the registers
    norm = lambda ins: Counter(re.sub(r"^(\S+) \d+$", r"\1 #", _REGNO.sub(_mask, i)) for i in ins)  # noqa: E731
    return "same instructions" if norm(a) == norm(b) else "different"


def pair(A, B, renames=()):
    """A, B: {name: instructions}; renames: (pattern, replacement) pairs applied in order to the names of A.
    -> [(name, class, instructions of A or None, of B or None)] sorted by name, a renamed symbol under its name in B."""
    for pat, repl in renames:
        A = {re.sub(pat, repl, n): ins for n, ins in A.items()}
    return [(n, classify(A.get(n), B.get(n)), A.get(n), B.get(n)) for n in sorted(set(A) | set(B))]


def main():
    args, renames = sys.argv[1:], []
    while args and args[0] == "--rename":
        renames.append((args[1], args[2]))
        args = args[3:]
    A, B, pats = by_name(symbols(args[0])), by_name(symbols(args[1])), args[2:]
    counts = Counter()
    for name, c, a, b in pair(A, B, renames):
        if pats and not any(p in name for p in pats):
            continue
        counts[c] += 1
        print("%-18s %6d %6d  %s" % (c, len(a or ()), len(b or ()), name))
    print("symbols %d: identical %d, same instructions %d, different %d"
          % (sum(counts.values()), counts["identical"], counts["same instructions"], counts["different"]))
    sys.exit(1 if counts["different"] else 0)


if __name__ == "__main__":
    main()

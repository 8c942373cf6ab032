// Cycle stamps of the sequential kernels (debug builds: -DTOLG_STAMPS, run through TOLG_HIP_LIB; tools/k2_stamps.py,
// tools/k3_stamps.py): one form for the backward sweeps, the rollouts and the fused launch's waves.  Included by
// tolg_kernels.hip inside namespace tolg, behind Params.
// TOLG_STAMP(st, k) adds the s_memtime ticks since the previous stamp to phase k of st.  Without TOLG_STAMPS the struct is
// empty, the macro and the flush are nothing: a step function takes its Stamps by reference in every build.  A stamped
// wave hands its sums to the caller through rows of the history arrays that no trajectory of a benchmark-sized batch
// stops at (row r of a [B][max_iter] history; tools/stamp_rows.py reads the numbers below).
#pragma once

enum {
  ST_BLOCK_ROLL = 5, ST_BLOCK_K2 = 7,  // the workgroup whose waves report: rollouts / backward sweeps
  ST_ROW_ROLL = 80,     // alpha_hist: the rollout chain (roll_step in k_rollout, roll_step_twist in wave 0 of k_rollout_lin)
  ST_ROW_HELPER = 81,   // alpha_hist: k_rollout_lin's helper h at row 81 + h: waiting, working
  ST_ROW_POSE = 83,     // alpha_hist: k_rollout_lin's pose wave
  ST_ROW_K2 = 28,       // mu_hist: the backward sweep's phases
  ST_ROW_K2_CLOCK = 29  // mu_hist: the sweep by s_memrealtime (100 MHz) and by s_memtime
};
template <int NP>
struct Stamps {
#ifdef TOLG_STAMPS
  unsigned long long acc[NP], t, t0, rt0;
  TOLG_DEV Stamps() {
    for (int k = 0; k < NP; k++) acc[k] = 0;
    rt0 = __builtin_amdgcn_s_memrealtime();
    t = t0 = __builtin_amdgcn_s_memtime();
  }
#endif
};
#ifdef TOLG_STAMPS
#define TOLG_STAMP(st, k) { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); (st).acc[k] += t_ - (st).t; (st).t = t_; __builtin_amdgcn_sched_barrier(0); }
#else
#define TOLG_STAMP(st, k)
#endif
// finer split of one phase of k_backward3 (-DTOLG_STAMPS -DTOLG_STAMPS2): a stamp that only the fine / only the coarse build takes
#ifdef TOLG_STAMPS2
#define TOLG_STAMP_FINE(st, k) TOLG_STAMP(st, k)
#define TOLG_STAMP_COARSE(st, k)
#else
#define TOLG_STAMP_FINE(st, k)
#define TOLG_STAMP_COARSE(st, k) TOLG_STAMP(st, k)
#endif
// `me`: this thread reports (one lane of workgroup ST_BLOCK_*).  A batch or a history too small to hold the row is refused:
// hist is [B][max_iter], the sums take row[0 .. NP) and, where asked for, clock_row[0 .. 2).
template <int NP>
TOLG_DEV void stamps_flush(const Params& P, const Stamps<NP>& st, bool me, double* hist, int row, int clock_row = -1) {
#ifdef TOLG_STAMPS
  if (!me || !hist || row >= P.B || clock_row >= P.B || P.max_iter < (NP > 2 ? NP : 2)) return;
  for (int k = 0; k < NP; k++) hist[(size_t)row * P.max_iter + k] = (double)st.acc[k];
  if (clock_row >= 0) {
    hist[(size_t)clock_row * P.max_iter + 0] = (double)(__builtin_amdgcn_s_memrealtime() - st.rt0);
    hist[(size_t)clock_row * P.max_iter + 1] = (double)(__builtin_amdgcn_s_memtime() - st.t0);
  }
#endif
}

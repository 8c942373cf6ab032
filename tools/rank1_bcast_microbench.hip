// The rank-1 measurement update of k_policy_covariance_est in isolation, with the column broadcast in its two candidate forms:
//   form 0  the row's LDS: lane c stores its column (12 doubles), one barrier, every lane reads the same twelve addresses
//   form 1  DPP moves: row_newbcast:c of each of the twelve values, on the two 32-bit halves (24 v_mov_b32_dpp; the way
//           quad_bcast moves a double), no LDS, no barrier
// Same plan as the kernel: one 16-lane row per trajectory, four rows per 64-thread block, lane j < 12 holds column j of a
// symmetric 12 x 12 P in registers; an update is  s = P[c][c] + V[c],  P[k][j] -= (P[k][c] * P[c][j]) / s  for every measured c.
// Between updates P is pulled back towards its start (P = 0.5 (P + P0)), so that it neither collapses nor the loop folds away.
// Prints ns per update (one measured coordinate, one row) for both forms at the kernel's grid, and whether the two forms end
// on the same bits.
//   hipcc --offload-arch=gfx950 -O3 -o tools/rank1_bcast_microbench tools/rank1_bcast_microbench.hip
//   tools/rank1_bcast_microbench [rows=4096] [knots=200] [mask=0x03f] [rounds=7]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int C>
__device__ __forceinline__ double row_bcast(double x) {  // value of x in lane C of this lane's 16-lane row
  constexpr int ctrl = 0x150 + C;  // row_newbcast:C
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, ctrl, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), ctrl, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

template <int FORM, int C>
__device__ __forceinline__ void update(double (&p)[12], double* T, int l, double vc) {
  double col[12];
  if constexpr (FORM == 0) {
    if (l == C) {
#pragma unroll
      for (int k = 0; k < 12; k++) T[12 * C + k] = p[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; k++) col[k] = T[12 * C + k];
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) col[k] = row_bcast<C>(p[k]);
  }
  const double is = 1.0 / (col[C] + vc), cj = p[C];
#pragma unroll
  for (int k = 0; k < 12; k++) p[k] -= (col[k] * cj) * is;
}

template <int FORM, int C = 0>
__device__ __forceinline__ void updates(double (&p)[12], double* T, int l, int mask, const double (&v)[12]) {
  if constexpr (C < 12) {
    if ((mask >> C) & 1) update<FORM, C>(p, T, l, v[C]);
    updates<FORM, C + 1>(p, T, l, mask, v);
  }
}

template <int FORM>
__global__ __launch_bounds__(64) void k_rank1(int rows, int knots, int mask, const double* __restrict__ P0,
                                              const double* __restrict__ V, double* __restrict__ out) {
  __shared__ double lds[4 * 144];
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  int b = blockIdx.x * 4 + g;
  const bool live = b < rows;
  if (!live) b = rows - 1;
  const int j = l < 12 ? l : 11;
  double* T = lds + g * 144;
  double p[12], p0[12], v[12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    p0[k] = P0[(size_t)b * 144 + (k <= j ? 12 * k + j : 12 * j + k)];
    p[k] = p0[k];
    v[k] = V[(size_t)b * 12 + k];
  }
  for (int i = 0; i < knots; i++) {
    updates<FORM>(p, T, l, mask, v);
    if constexpr (FORM == 0) __syncthreads();  // the slots are rewritten by the next knot
#pragma unroll
    for (int k = 0; k < 12; k++) p[k] = 0.5 * (p[k] + p0[k]);
  }
  if (live && l < 12) {
#pragma unroll
    for (int k = 0; k < 12; k++) out[(size_t)b * 144 + 12 * k + l] = p[k];
  }
}

int main(int argc, char** argv) {
  const int rows = argc > 1 ? atoi(argv[1]) : 4096, knots = argc > 2 ? atoi(argv[2]) : 200;
  const int mask = argc > 3 ? (int)strtol(argv[3], nullptr, 0) : 0x03f, rounds = argc > 4 ? atoi(argv[4]) : 7;
  if (rows < 1 || knots < 1 || mask < 0 || mask > 0xfff || rounds < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
  int nm = 0;
  for (int c = 0; c < 12; c++) nm += (mask >> c) & 1;
  // a seeded symmetric positive definite P0 per row (diagonally dominant), V = its diagonal
  std::vector<double> hP((size_t)rows * 144), hV((size_t)rows * 12);
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  for (int b = 0; b < rows; b++) {
    double* M = &hP[(size_t)b * 144];
    for (int r = 0; r < 12; r++)
      for (int c = r; c < 12; c++) M[12 * r + c] = M[12 * c + r] = r == c ? 2.0 + rnd() : 0.1 * (rnd() - 0.5);
    for (int r = 0; r < 12; r++) hV[(size_t)b * 12 + r] = M[13 * r];
  }
  double *dP, *dV, *dO[2];
  CHECK(hipMalloc(&dP, hP.size() * 8)); CHECK(hipMalloc(&dV, hV.size() * 8));
  CHECK(hipMalloc(&dO[0], hP.size() * 8)); CHECK(hipMalloc(&dO[1], hP.size() * 8));
  CHECK(hipMemcpy(dP, hP.data(), hP.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dV, hV.data(), hV.size() * 8, hipMemcpyHostToDevice));
  const dim3 grid((unsigned)((rows + 3) / 4)), block(64);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  std::vector<float> ms[2];
  for (int r = -1; r < rounds; r++) {  // round -1: warm-up
    for (int t = 0; t < 2; t++) {
      const int f = (r + t) & 1;  // the forms alternate in who goes first
      CHECK(hipEventRecord(e0));
      if (f == 0) hipLaunchKernelGGL(k_rank1<0>, grid, block, 0, 0, rows, knots, mask, dP, dV, dO[0]);
      else hipLaunchKernelGGL(k_rank1<1>, grid, block, 0, 0, rows, knots, mask, dP, dV, dO[1]);
      CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
      float x; CHECK(hipEventElapsedTime(&x, e0, e1));
      if (r >= 0) ms[f].push_back(x);
    }
  }
  CHECK(hipGetLastError());
  std::vector<double> h0(hP.size()), h1(hP.size());
  CHECK(hipMemcpy(h0.data(), dO[0], h0.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(h1.data(), dO[1], h1.size() * 8, hipMemcpyDeviceToHost));
  bool same = memcmp(h0.data(), h1.data(), h0.size() * 8) == 0, sym = true, fin = true;
  for (int b = 0; b < rows && sym; b++)
    for (int r = 0; r < 12; r++)
      for (int c = 0; c < 12; c++) {
        if (h0[(size_t)b * 144 + 12 * r + c] != h0[(size_t)b * 144 + 12 * c + r]) sym = false;
        if (!(h0[(size_t)b * 144 + 12 * r + c] == h0[(size_t)b * 144 + 12 * r + c])) fin = false;
      }
  const char* name[2] = {"row's LDS (12 ds_read_b64 + barrier)", "DPP moves (24 v_mov_b32_dpp)"};
  printf("rank-1 update broadcast, rows %d, knots %d, mask 0x%03x (%d measured), %d rounds, grid %u x 64\n", rows, knots, mask, nm,
         rounds, grid.x);
  double med[2];
  for (int f = 0; f < 2; f++) {
    std::sort(ms[f].begin(), ms[f].end());
    med[f] = ms[f][ms[f].size() / 2];
    printf("form %d  %-38s  %8.4f ms per launch (min %.4f, max %.4f)  %7.2f ns per update on the chain\n", f, name[f], med[f],
           ms[f].front(), ms[f].back(), nm ? med[f] * 1e6 / ((double)knots * nm) : 0.0);
  }
  printf("DPP / LDS = %.3f; the two forms end on the same bits: %s; symmetric to the bit: %s; finite: %s\n", med[1] / med[0],
         same ? "yes" : "NO", sym ? "yes" : "NO", fin ? "yes" : "NO");
  return same && sym && fin ? 0 : 1;
}

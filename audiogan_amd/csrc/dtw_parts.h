// dtw_parts.h -- the dynamic-time-warping recursion, once: what dtw_cost_kernel (evalalign.hip), dtw_pairs_wave_kernel and
// dtw_pairs_wg_kernel (evalpairs.hip) and dtw_align_kernel (dtwalign.hip) share.  Each of those kernels is its own index and
// count set-up, a fill, a row load, one barrier, one sweep and its own store; the cell and the step loop exist only here, so
// the totals of ag_dtw_cost, ag_dtw_pairs and ag_dtw_align have the same bits for the same two sequences because they are
// the same code.  Device-only.
//
// The scheme.  D(i, j) = min(D(i-1, j) + d, D(i, j-1) + d, D(i-1, j-1) + 2 d), D(0, 0) = 2 d, d = d(i, j) the Euclidean
// distance between the 12 cepstral coefficients of the two frames.  Thread i owns row i of the cost matrix (frame i of the
// rows side, its coefficients in registers; the columns side sits in LDS) and walks the n + m - 1 anti-diagonals: at step
// s it is at column j = s - i.  Of the three predecessors, D(i, j-1) is the thread's own previous value; D(i-1, j) is thread i-1's
// value of the previous step and D(i-1, j-1) its value of the step before - what this thread received one step earlier.
// So a step costs one shuffle.  In a workgroup of several waves, lane 0 of a wave takes its neighbour's value from LDS,
// where lane 63 of every wave leaves it: two slots in turn, so ONE barrier per step orders the write of step s, its read in
// step s + 1 and the overwrite in step s + 2.  The trip count n + m - 1 is the same for every thread of the workgroup and no
// thread leaves before the last barrier.  A single wave exchanges nothing with another: its sweep has no barrier at all.
// Which side supplies the rows does not show in the bits: min is commutative and the local cost is the same sum of the same
// squares either way, so dtw(a, b) and dtw(b, a) are equal without a choice of sides.
#pragma once
#include "common.h"

#define DTW_MAX 1024         // frames a side
#define DTW_Q 12             // coefficients: columns 1..12 ...
#define DTW_ROW 16           // ... of a 16-float row
#define DTW_PACK 16          // predecessor codes per 32-bit word

// sequence k's frame count, clamped to [1, capacity]; without a count list every sequence is full
__device__ __forceinline__ int dtw_count(const int32_t* __restrict__ nf, int k, int F) {
  return min(max(nf ? nf[k] : F, 1), F);
}

// the columns side: the m * 12 coefficients of sequence k of a bank of capacity F into sb, by nt threads of which this is t.
// nt keeps the caller's type: blockDim.x is unsigned and a stride of that type compiles to the plain loop, a constant int
// to the unrolled one - each as its kernel had it.
template <class Stride>
__device__ __forceinline__ void dtw_fill_cols(float* sb, const float* __restrict__ bank, int k, int F, int m, int t,
                                              Stride nt) {
  const float* src = bank + (int64_t)k * F * DTW_ROW;
  for (int e = t; e < m * DTW_Q; e += nt) {
    const int j = e / DTW_Q, q = e - j * DTW_Q;
    sb[e] = src[j * DTW_ROW + 1 + q];
  }
}

// the rows side: the coefficients of row min(i, n - 1) of sequence k (idle threads: a row that exists)
__device__ __forceinline__ void dtw_load_row(float (&a)[DTW_Q], const float* __restrict__ bank, int k, int F, int i, int n) {
  const float* src = bank + ((int64_t)k * F + min(i, n - 1)) * DTW_ROW + 1;
#pragma unroll
  for (int q = 0; q < DTW_Q; ++q) a[q] = src[q];
}

// One cell: row i's at step s, D(i, j) with j = s - i, from the columns side in sb and the three neighbours.  With DEC also
// the predecessor the path back takes: 0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1), the first in that order whose candidate
// equals the minimum; on row 0 only 2 exists, in column 0 only 1.  The value does not depend on DEC.  (It is given s and
// forms j itself: that keeps "i == 0 && s == i" in sight of the sweep's loop, whose steps after the first cannot be (0, 0).)
template <bool DEC>
__device__ __forceinline__ float dtw_cell(const float (&a)[DTW_Q], const float* sb, int i, int s, float up, float cur,
                                          float diag, uint32_t& dec) {
  const int j = s - i;
  const f32x4* r = reinterpret_cast<const f32x4*>(sb + j * DTW_Q);
  float ss = 0.f;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const f32x4 bv = r[v];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float df = a[4 * v + q] - bv[q];
      ss = fmaf(df, df, ss);
    }
  }
  const float d = sqrtf(ss);
  const float inf = __builtin_inff();
  float best;
  if (i == 0 && j == 0) {
    best = d + d;
    if (DEC) dec = 2u;
  } else {
    float cu = inf, cd = inf;
    best = inf;
    if (i > 0) best = cu = up + d;
    if (j > 0) best = fminf(best, cur + d);
    if (i > 0 && j > 0) best = fminf(best, cd = diag + (d + d));
    if (DEC) dec = i == 0 ? 2u : (j == 0 ? 1u : (cd == best ? 0u : (cu == best ? 1u : 2u)));
  }
  return best;
}

// The sweep of a workgroup: thread i of ag_roundup(capacity, 64), every one of which calls it (idle rows included: they
// shuffle, hand over and wait at the barriers).  edge is the two-slot hand-off between waves.  After each cell of its row
// the thread calls hook(j, dec), dec being the cell's predecessor code when DEC is set.  Returns the thread's last value:
// D(n-1, m-1) in thread n - 1.
template <bool DEC, class Hook>
__device__ __forceinline__ float dtw_sweep_wg(const float (&a)[DTW_Q], const float* sb, float (&edge)[2][16], int i, int n,
                                              int m, Hook hook) {
  const int lane = i & 63, w = i >> 6;
  const float inf = __builtin_inff();
  float cur = inf, diag = inf;
  const int steps = n + m - 1;
  for (int s = 0; s < steps; ++s) {
    float up = __shfl_up(cur, 1, 64);
    if (lane == 0 && w > 0 && s > 0) up = edge[(s - 1) & 1][w - 1];
    const int j = s - i;
    if (i < n && j >= 0 && j < m) {
      uint32_t dec = 0;
      cur = dtw_cell<DEC>(a, sb, i, s, up, cur, diag, dec);
      hook(j, dec);
    }
    diag = up;
    if (lane == 63) edge[s & 1][w] = cur;
    __syncthreads();
  }
  return cur;
}

// ... for the total alone
__device__ __forceinline__ float dtw_sweep_wg(const float (&a)[DTW_Q], const float* sb, float (&edge)[2][16], int i, int n,
                                              int m) {
  return dtw_sweep_wg<false>(a, sb, edge, i, n, m, [](int, uint32_t) {});
}

// The sweep of a single wave (n <= 64), lane = row: no barrier.
__device__ __forceinline__ float dtw_sweep_wave(const float (&a)[DTW_Q], const float* sb, int lane, int n, int m) {
  const float inf = __builtin_inff();
  float cur = inf, diag = inf;
  const int steps = n + m - 1;
  for (int s = 0; s < steps; ++s) {
    const float up = __shfl_up(cur, 1, 64);
    const int j = s - lane;
    if (lane < n && j >= 0 && j < m) {
      uint32_t dec = 0;
      cur = dtw_cell<false>(a, sb, lane, s, up, cur, diag, dec);
    }
    diag = up;
  }
  return cur;
}

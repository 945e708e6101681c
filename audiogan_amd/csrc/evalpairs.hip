// evalpairs.hip -- ag_dtw_pairs: the dynamic-time-warping total of ag_dtw_cost (evalalign.hip) for MANY pairs drawn from two
// banks of cepstral sequences, by index lists or as the cross product (audiogan_amd/evaluate.py: Evaluator(crossed=True,
// draws=k), aligned_distance_matrix; contract in include/audiogan_hip.h).  No gathered copies of the banks, LDS sized by the
// capacities, and the bits of ag_dtw_cost for the same two sequences: the local cost and the three candidates are the same
// expressions in the same order.  fp32 whatever ag_set_precision says, no atomics, no dependency between workgroups, trip
// counts n + m - 1 <= 2047: two runs give the same bits.
//
// Two forms, chosen on the host from the CAPACITIES (never from device values):
//   wave form       min(Fa, Fb) <= 64 and max(Fa, Fb) <= 256.  One wave per pair, four pairs per 256-thread workgroup.  The
//                   side of at most 64 frames is the rows side (lane i owns row i, its 12 coefficients in registers); the
//                   other side sits in the wave's own slice of dynamic LDS (Fc * 48 bytes).  D(i-1, j) is __shfl_up of
//                   the previous step's value, D(i-1, j-1) what the lane received one step earlier: a wave exchanges
//                   nothing with another, so the step loop has no barrier.  One __syncthreads() orders the fill before
//                   the first read; every wave of the workgroup reaches it, those of a partial last workgroup included.
//                   When a is the longer side the host swaps the roles (ag_dtw_cost documents that the bits do not
//                   depend on the sides) and the kernel maps the pair number back, so out keeps its layout.
//   workgroup form  everything else up to 1024 frames a side: the scheme of dtw_cost_kernel - a thread per row of a, lane
//                   63 of every wave leaves its value in one of two LDS slots for lane 0 of the next, one barrier per step -
//                   with pair indices and dynamic LDS of Fb * 48 bytes.
#include "common.h"

#define DP_MAX 1024
#define DP_Q 12              // columns 1..12 of a 16-float row
#define DP_ROW 16
#define DP_WAVE_ROWS 64      // the wave form's rows side
#define DP_WAVE_COLS 256     // ... and its columns side: 4 slices of 256 * 48 bytes are 48 KB
#define DP_PER_WG 4          // pairs (waves) per workgroup of the wave form

// the pair's sequences: explicit lists (given in rows / columns order), or pair p = (p / cross_nb, p % cross_nb) of the
// cross product in a / b order, exchanged when the host swapped the sides.  Clamped: a wrong index is a wrong pair, never
// an address outside the banks.
__device__ __forceinline__ void dp_pair(const int32_t* __restrict__ ir, const int32_t* __restrict__ ic, int p, int cross_nb,
                                        int swapped, int Nr, int Nc, int& ri, int& ci) {
  if (ir) {
    ri = ir[p];
    ci = ic[p];
  } else {
    const int ai = p / cross_nb, bi = p - ai * cross_nb;
    ri = swapped ? bi : ai;
    ci = swapped ? ai : bi;
  }
  ri = min(max(ri, 0), Nr - 1);
  ci = min(max(ci, 0), Nc - 1);
}

// one cell: the expressions of dtw_cost_kernel, in its order
__device__ __forceinline__ float dp_cell(const float (&a)[DP_Q], const float* __restrict__ col, int i, int j, float up,
                                         float cur, float diag) {
  const f32x4* r = reinterpret_cast<const f32x4*>(col);
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
  float best;
  if (i == 0 && j == 0) {
    best = d + d;
  } else {
    best = __builtin_inff();
    if (i > 0) best = up + d;
    if (j > 0) best = fminf(best, cur + d);
    if (i > 0 && j > 0) best = fminf(best, diag + (d + d));
  }
  return best;
}

__global__ __launch_bounds__(64 * DP_PER_WG) void dtw_pairs_wave_kernel(
    const float* __restrict__ cr, const int32_t* __restrict__ nfr, int Nr, int Fr, const float* __restrict__ cc,
    const int32_t* __restrict__ nfc, int Nc, int Fc, const int32_t* __restrict__ ir, const int32_t* __restrict__ ic,
    float* __restrict__ out, int P, int cross_nb, int swapped) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = blockIdx.x * DP_PER_WG + w;
  const bool live = p < P;          // (wave-uniform)
  float* sb = dp_lds + w * Fc * DP_Q;
  int n = 1, m = 1;
  float a[DP_Q];
#pragma unroll
  for (int q = 0; q < DP_Q; ++q) a[q] = 0.f;
  if (live) {
    int ri, ci;
    dp_pair(ir, ic, p, cross_nb, swapped, Nr, Nc, ri, ci);
    n = min(max(nfr ? nfr[ri] : Fr, 1), min(Fr, DP_WAVE_ROWS));
    m = min(max(nfc ? nfc[ci] : Fc, 1), Fc);
    const float* src = cc + (int64_t)ci * Fc * DP_ROW;
    for (int e = lane; e < m * DP_Q; e += 64) {
      const int j = e / DP_Q, q = e - j * DP_Q;
      sb[e] = src[j * DP_ROW + 1 + q];
    }
    src = cr + ((int64_t)ri * Fr + min(lane, n - 1)) * DP_ROW + 1;          // (idle lanes: a row that exists)
#pragma unroll
    for (int q = 0; q < DP_Q; ++q) a[q] = src[q];
  }
  __syncthreads();          // the only barrier: every wave of the workgroup is here, live or not
  if (!live) return;
  const float inf = __builtin_inff();
  float cur = inf, diag = inf;
  const int steps = n + m - 1;
  for (int s = 0; s < steps; ++s) {
    const float up = __shfl_up(cur, 1, 64);
    const int j = s - lane;
    if (lane < n && j >= 0 && j < m) cur = dp_cell(a, sb + j * DP_Q, lane, j, up, cur, diag);
    diag = up;
  }
  if (lane == n - 1) out[p] = cur;
}

__global__ __launch_bounds__(1024) void dtw_pairs_wg_kernel(const float* __restrict__ ca, const int32_t* __restrict__ nfa,
                                                            int Na, int Fa, const float* __restrict__ cb,
                                                            const int32_t* __restrict__ nfb, int Nb, int Fb,
                                                            const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                            float* __restrict__ out, int cross_nb) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];          // Fb * DP_Q floats
  __shared__ float edge[2][16];          // (128 bytes: the dynamic region stays 16-byte aligned)
  float* sb = dp_lds;
  const int p = blockIdx.x, i = threadIdx.x, lane = i & 63, w = i >> 6;
  int ai, bi;
  dp_pair(ia, ib, p, cross_nb, 0, Na, Nb, ai, bi);
  const int n = min(max(nfa ? nfa[ai] : Fa, 1), Fa), m = min(max(nfb ? nfb[bi] : Fb, 1), Fb);
  {
    const float* src = cb + (int64_t)bi * Fb * DP_ROW;
    for (int e = i; e < m * DP_Q; e += blockDim.x) {
      const int j = e / DP_Q, q = e - j * DP_Q;
      sb[e] = src[j * DP_ROW + 1 + q];
    }
  }
  float a[DP_Q];
  {
    const float* src = ca + ((int64_t)ai * Fa + min(i, n - 1)) * DP_ROW + 1;          // (idle threads: a row that exists)
#pragma unroll
    for (int q = 0; q < DP_Q; ++q) a[q] = src[q];
  }
  __syncthreads();
  const float inf = __builtin_inff();
  float cur = inf, diag = inf;
  const int steps = n + m - 1;          // (the same for every thread: no thread leaves before the last barrier)
  for (int s = 0; s < steps; ++s) {
    float up = __shfl_up(cur, 1, 64);
    if (lane == 0 && w > 0 && s > 0) up = edge[(s - 1) & 1][w - 1];
    const int j = s - i;
    if (i < n && j >= 0 && j < m) cur = dp_cell(a, sb + j * DP_Q, i, j, up, cur, diag);
    diag = up;
    if (lane == 63) edge[s & 1][w] = cur;
    __syncthreads();
  }
  if (i == n - 1) out[p] = cur;
}

extern "C" int ag_dtw_pairs(const float* cep_a, const int32_t* nf_a, int Na, int Fa, const float* cep_b, const int32_t* nf_b,
                            int Nb, int Fb, const int32_t* ia, const int32_t* ib, float* out, int P, void* stream) {
  AG_REQUIRE(cep_a && cep_b && out, "ag_dtw_pairs: null cep_a, cep_b or out");
  AG_REQUIRE((ia != nullptr) == (ib != nullptr), "ag_dtw_pairs: ia and ib are both given or both NULL");
  AG_REQUIRE(Na >= 1 && Na <= 65535 && Nb >= 1 && Nb <= 65535, "ag_dtw_pairs: banks of 1..65535 sequences (got %d, %d)", Na,
             Nb);
  AG_REQUIRE(P > 0 && P <= (1 << 24), "ag_dtw_pairs: 1..2^24 pairs (got %d)", P);
  AG_REQUIRE(ia || (int64_t)P == (int64_t)Na * Nb, "ag_dtw_pairs: without index lists P is Na * Nb = %lld (got %d)",
             (long long)Na * Nb, P);
  AG_REQUIRE(Fa >= 1 && Fa <= DP_MAX && Fb >= 1 && Fb <= DP_MAX,
             "ag_dtw_pairs: sequences of 1..%d frames (got capacities %d, %d)", DP_MAX, Fa, Fb);
  const int lo = Fa < Fb ? Fa : Fb, hi = Fa < Fb ? Fb : Fa;
  if (lo <= DP_WAVE_ROWS && hi <= DP_WAVE_COLS) {
    const int swapped = Fa > DP_WAVE_ROWS;          // the rows side has at most 64 frames
    const float* cr = swapped ? cep_b : cep_a;
    const float* cc = swapped ? cep_a : cep_b;
    const int32_t* nfr = swapped ? nf_b : nf_a;
    const int32_t* nfc = swapped ? nf_a : nf_b;
    const int Nr = swapped ? Nb : Na, Nc = swapped ? Na : Nb, Fr = swapped ? Fb : Fa, Fc = swapped ? Fa : Fb;
    ag_note_kernel("dtw_pairs_wave_kernel");
    hipLaunchKernelGGL(dtw_pairs_wave_kernel, dim3(ag_cdiv(P, DP_PER_WG)), dim3(64 * DP_PER_WG),
                       (size_t)DP_PER_WG * Fc * DP_Q * sizeof(float), (hipStream_t)stream, cr, nfr, Nr, Fr, cc, nfc, Nc, Fc,
                       swapped ? ib : ia, swapped ? ia : ib, out, P, Nb, swapped);
  } else {
    ag_note_kernel("dtw_pairs_wg_kernel");
    hipLaunchKernelGGL(dtw_pairs_wg_kernel, dim3(P), dim3(ag_roundup(Fa, AG_WAVE)), (size_t)Fb * DP_Q * sizeof(float),
                       (hipStream_t)stream, cep_a, nf_a, Na, Fa, cep_b, nf_b, Nb, Fb, ia, ib, out, Nb);
  }
  AG_CHECK_LAUNCH("ag_dtw_pairs");
  return AG_OK;
}

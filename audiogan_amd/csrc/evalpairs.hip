// evalpairs.hip -- ag_dtw_pairs: the dynamic-time-warping total of ag_dtw_cost (evalalign.hip) for MANY pairs drawn from two
// banks of cepstral sequences, by index lists or as the cross product (audiogan_amd/evaluate.py: Evaluator(crossed=True,
// draws=k), aligned_distance_matrix; contract in include/audiogan_hip.h).  No gathered copies of the banks and LDS sized by
// the capacities; the recursion is dtw_parts.h's, which is why the bits are ag_dtw_cost's.  fp32 whatever ag_set_precision
// says, no atomics, no dependency between workgroups, trip counts n + m - 1 <= 2047: two runs give the same bits.
//
// Two forms, chosen on the host from the CAPACITIES (never from device values):
//   wave form       min(Fa, Fb) <= 64 and max(Fa, Fb) <= 256.  One wave per pair, four pairs per 256-thread workgroup, the
//                   wave sweep.  The side of at most 64 frames is the rows side; the other sits in the wave's own slice of
//                   dynamic LDS (Fc * 48 bytes).  One __syncthreads() orders the fill before the first read; every wave of
//                   the workgroup reaches it, those of a partial last workgroup included.  When a is the longer side the
//                   host swaps the roles (the sides commute) and the kernel maps the pair number back, so out keeps its
//                   layout.
//   workgroup form  everything else up to 1024 frames a side: a thread per row of a, the workgroup sweep, with pair indices
//                   and dynamic LDS of Fb * 48 bytes.
#include "common.h"
#include "dtw_parts.h"

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

__global__ __launch_bounds__(64 * DP_PER_WG) void dtw_pairs_wave_kernel(
    const float* __restrict__ cr, const int32_t* __restrict__ nfr, int Nr, int Fr, const float* __restrict__ cc,
    const int32_t* __restrict__ nfc, int Nc, int Fc, const int32_t* __restrict__ ir, const int32_t* __restrict__ ic,
    float* __restrict__ out, int P, int cross_nb, int swapped) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = blockIdx.x * DP_PER_WG + w;
  const bool live = p < P;          // (wave-uniform)
  float* sb = dp_lds + w * Fc * DTW_Q;
  int n = 1, m = 1;
  float a[DTW_Q];
#pragma unroll
  for (int q = 0; q < DTW_Q; ++q) a[q] = 0.f;
  if (live) {
    int ri, ci;
    dp_pair(ir, ic, p, cross_nb, swapped, Nr, Nc, ri, ci);
    n = min(dtw_count(nfr, ri, Fr), DP_WAVE_ROWS);
    m = dtw_count(nfc, ci, Fc);
    dtw_fill_cols(sb, cc, ci, Fc, m, lane, 64);
    dtw_load_row(a, cr, ri, Fr, lane, n);
  }
  __syncthreads();          // the only barrier: every wave of the workgroup is here, live or not
  if (!live) return;
  const float cur = dtw_sweep_wave(a, sb, lane, n, m);
  if (lane == n - 1) out[p] = cur;
}

__global__ __launch_bounds__(1024) void dtw_pairs_wg_kernel(const float* __restrict__ ca, const int32_t* __restrict__ nfa,
                                                            int Na, int Fa, const float* __restrict__ cb,
                                                            const int32_t* __restrict__ nfb, int Nb, int Fb,
                                                            const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                            float* __restrict__ out, int cross_nb) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];          // Fb * DTW_Q floats
  __shared__ float edge[2][16];          // (128 bytes: the dynamic region stays 16-byte aligned)
  const int p = blockIdx.x, i = threadIdx.x;
  int ai, bi;
  dp_pair(ia, ib, p, cross_nb, 0, Na, Nb, ai, bi);
  const int n = dtw_count(nfa, ai, Fa), m = dtw_count(nfb, bi, Fb);
  dtw_fill_cols(dp_lds, cb, bi, Fb, m, i, blockDim.x);
  float a[DTW_Q];
  dtw_load_row(a, ca, ai, Fa, i, n);
  __syncthreads();
  const float cur = dtw_sweep_wg(a, dp_lds, edge, i, n, m);
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
  AG_REQUIRE(Fa >= 1 && Fa <= DTW_MAX && Fb >= 1 && Fb <= DTW_MAX,
             "ag_dtw_pairs: sequences of 1..%d frames (got capacities %d, %d)", DTW_MAX, Fa, Fb);
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
                       (size_t)DP_PER_WG * Fc * DTW_Q * sizeof(float), (hipStream_t)stream, cr, nfr, Nr, Fr, cc, nfc, Nc, Fc,
                       swapped ? ib : ia, swapped ? ia : ib, out, P, Nb, swapped);
  } else {
    ag_note_kernel("dtw_pairs_wg_kernel");
    hipLaunchKernelGGL(dtw_pairs_wg_kernel, dim3(P), dim3(ag_roundup(Fa, AG_WAVE)), (size_t)Fb * DTW_Q * sizeof(float),
                       (hipStream_t)stream, cep_a, nf_a, Na, Fa, cep_b, nf_b, Nb, Fb, ia, ib, out, Nb);
  }
  AG_CHECK_LAUNCH("ag_dtw_pairs");
  return AG_OK;
}

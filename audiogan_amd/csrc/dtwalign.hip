// dtwalign.hip -- ag_dtw_align: the dynamic-time-warping recursion of ag_dtw_cost (evalalign.hip) with the PATH, for
// cutting a transcribed utterance into words against a reference sequence (audiogan_amd/align.py; contract in
// include/audiogan_hip.h).  fp32 whatever ag_set_precision says, no atomics, no dependency between workgroups: two runs give
// the same bits.
//
// Forward.  The step loop is dtw_cost_kernel's: one workgroup per pair, thread i owns row i (frame i of a, its 12
// coefficients in registers; b's sit in LDS), one shuffle and one barrier per anti-diagonal, the same fmaf chain, sqrtf,
// fminf order and d + d, so the total has ag_dtw_cost's bits.  Beside the value each cell yields the predecessor the path
// back takes: 0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1), the first in that order whose candidate equals the minimum (on
// row 0 only 2 exists, in column 0 only 1).  Thread i packs the codes of 16 consecutive columns of its row into one
// 32-bit word and stores it when column 16 k + 15 or the row's last column is done: word k of row i lies at
// ws[i * ceil(Fb / 16) + k].  One 4-byte vector store per 16 steps and thread; at most 256 KB per pair.
//
// Walk back.  After the loop's last barrier every cell is final; __threadfence_block() and one more __syncthreads() make the
// workgroup's own stores visible to thread 0 (all waves of a workgroup share their CU's vector cache, the stores write
// through it, and the words are read with vector loads - never through the scalar cache, which is not kept coherent with
// them).  Thread 0 walks from (n-1, m-1) to (0, 0), at most n + m - 2 moves, holding the word it read last (a run of moves
// to the left inside one word costs one load), and leaves per column the first and the last row on the path in LDS; after a
// barrier the workgroup writes lo[b, j], hi[b, j] for j < m in whole rows.  A code that is no move from its cell (row 0,
// column 0) is never followed: the walk cannot leave the matrix whatever the workspace holds.
#include "common.h"

#define DA_MAX 1024
#define DA_Q 12              // columns 1..12 of a 16-float row
#define DA_ROW 16
#define DA_PACK 16           // cells per 32-bit word

static inline int64_t da_ws_bytes(int Fa, int Fb) { return (int64_t)Fa * ag_cdiv(Fb, DA_PACK) * 4; }

template <bool WALK>
__global__ __launch_bounds__(1024) void dtw_align_kernel(const float* __restrict__ ca, const int32_t* __restrict__ nfa,
                                                         const float* __restrict__ cb, const int32_t* __restrict__ nfb,
                                                         float* __restrict__ total, int32_t* __restrict__ lo,
                                                         int32_t* __restrict__ hi, uint32_t* ws, int Fa, int Fb) {
  __shared__ __attribute__((aligned(16))) float sb[DA_MAX * DA_Q];
  __shared__ float edge[2][16];
  __shared__ int32_t slo[DA_MAX], shi[DA_MAX];
  const int b = blockIdx.x, i = threadIdx.x, lane = i & 63, w = i >> 6;
  const int n = min(max(nfa ? nfa[b] : Fa, 1), Fa), m = min(max(nfb ? nfb[b] : Fb, 1), Fb);
  const int W = (Fb + DA_PACK - 1) / DA_PACK;
  uint32_t* wsp = ws + (int64_t)b * Fa * W;
  {
    const float* src = cb + (int64_t)b * Fb * DA_ROW;
    for (int e = i; e < m * DA_Q; e += blockDim.x) {
      const int j = e / DA_Q, q = e - j * DA_Q;
      sb[e] = src[j * DA_ROW + 1 + q];
    }
  }
  float a[DA_Q];
  {
    const float* src = ca + ((int64_t)b * Fa + min(i, n - 1)) * DA_ROW + 1;          // (idle threads: a row that exists)
#pragma unroll
    for (int q = 0; q < DA_Q; ++q) a[q] = src[q];
  }
  __syncthreads();
  const float inf = __builtin_inff();
  float cur = inf, diag = inf;
  uint32_t word = 0;
  const int steps = n + m - 1;
  for (int s = 0; s < steps; ++s) {
    float up = __shfl_up(cur, 1, 64);
    if (lane == 0 && w > 0 && s > 0) up = edge[(s - 1) & 1][w - 1];
    const int j = s - i;
    if (i < n && j >= 0 && j < m) {
      const f32x4* r = reinterpret_cast<const f32x4*>(sb + j * DA_Q);
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
      uint32_t dec;
      if (i == 0 && j == 0) {
        best = d + d;
        dec = 2u;
      } else {          // (the values exactly as dtw_cost_kernel forms them)
        float cu = inf, cd = inf;
        best = inf;
        if (i > 0) best = cu = up + d;
        if (j > 0) best = fminf(best, cur + d);
        if (i > 0 && j > 0) best = fminf(best, cd = diag + (d + d));
        dec = i == 0 ? 2u : (j == 0 ? 1u : (cd == best ? 0u : (cu == best ? 1u : 2u)));
      }
      cur = best;
      word |= dec << (2 * (j & (DA_PACK - 1)));
      if ((j & (DA_PACK - 1)) == DA_PACK - 1 || j == m - 1) {
        wsp[i * W + (j >> 4)] = word;
        word = 0;
      }
    }
    diag = up;
    if (lane == 63) edge[s & 1][w] = cur;
    __syncthreads();
  }
  if (i == n - 1) total[b] = cur;
  if (!WALK) return;          // (the profiling tool's forward-only variant; the whole workgroup)

  __threadfence_block();
  __syncthreads();
  if (i == 0) {
    const uint32_t* rd = wsp;
    int ci = n - 1, cj = m - 1, hr = -1, hk = -1;
    uint32_t held = 0;
    shi[cj] = ci;
    for (int t = 0; t < steps - 1 && (ci | cj) != 0; ++t) {
      uint32_t dec;
      if (ci == 0) {
        dec = 2u;
      } else if (cj == 0) {
        dec = 1u;
      } else {
        if (ci != hr || (cj >> 4) != hk) {
          hr = ci;
          hk = cj >> 4;
          // (a relaxed workgroup-scope load is an ordinary vector load that the compiler may neither hoist nor scalarise)
          held = __hip_atomic_load(rd + ci * W + hk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        dec = (held >> (2 * (cj & (DA_PACK - 1)))) & 3u;
      }
      if (dec == 1u) {
        --ci;
      } else {
        slo[cj] = ci;
        if (dec == 0u) --ci;
        --cj;
        shi[cj] = ci;
      }
    }
    slo[0] = 0;
  }
  __syncthreads();
  for (int j = i; j < m; j += blockDim.x) {
    lo[(int64_t)b * Fb + j] = slo[j];
    hi[(int64_t)b * Fb + j] = shi[j];
  }
}

extern "C" int64_t ag_dtw_align_ws(int Fa, int Fb) {
  if (Fa < 1 || Fb < 1 || Fa > DA_MAX || Fb > DA_MAX) return 0;
  return da_ws_bytes(Fa, Fb);
}

static int da_launch(bool walk, const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b,
                     float* total, int32_t* lo, int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb, void* stream) {
  AG_REQUIRE(cep_a && cep_b && total && lo && hi && ws && B > 0, "ag_dtw_align: bad args");
  AG_REQUIRE(Fa >= 1 && Fb >= 1 && Fa <= DA_MAX && Fb <= DA_MAX,
             "ag_dtw_align: sequences of 1 to %d frames (got capacities %d, %d)", DA_MAX, Fa, Fb);
  AG_REQUIRE(ws_bytes >= (int64_t)B * da_ws_bytes(Fa, Fb), "ag_dtw_align: workspace of %lld bytes, needs %lld",
             (long long)ws_bytes, (long long)((int64_t)B * da_ws_bytes(Fa, Fb)));
  ag_note_kernel("dtw_align_kernel");
  const dim3 grid(B), block(ag_roundup(Fa, AG_WAVE));
  if (walk)
    hipLaunchKernelGGL(dtw_align_kernel<true>, grid, block, 0, (hipStream_t)stream, cep_a, nf_a, cep_b, nf_b, total, lo, hi,
                       (uint32_t*)ws, Fa, Fb);
  else
    hipLaunchKernelGGL(dtw_align_kernel<false>, grid, block, 0, (hipStream_t)stream, cep_a, nf_a, cep_b, nf_b, total, lo, hi,
                       (uint32_t*)ws, Fa, Fb);
  AG_CHECK_LAUNCH("ag_dtw_align");
  return AG_OK;
}

extern "C" int ag_dtw_align(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b, float* total,
                            int32_t* lo, int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb, void* stream) {
  return da_launch(true, cep_a, nf_a, cep_b, nf_b, total, lo, hi, ws, ws_bytes, B, Fa, Fb, stream);
}

// the forward pass alone (decisions recorded, lo / hi not written): what tools/prof_dtwalign.py times to split the cost
extern "C" int ag_dtw_align_forward(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b,
                                    float* total, int32_t* lo, int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb,
                                    void* stream) {
  return da_launch(false, cep_a, nf_a, cep_b, nf_b, total, lo, hi, ws, ws_bytes, B, Fa, Fb, stream);
}

// dtwalign.hip -- ag_dtw_align: the dynamic-time-warping recursion of ag_dtw_cost (evalalign.hip) with the PATH, for
// cutting a transcribed utterance into words against a reference sequence (audiogan_amd/align.py; contract in
// include/audiogan_hip.h).  fp32 whatever ag_set_precision says, no atomics, no dependency between workgroups: two runs give
// the same bits.
//
// Forward.  One workgroup per pair, a's frames the rows; the recursion is dtw_parts.h's workgroup sweep with the predecessor
// codes on, which is why the total has ag_dtw_cost's bits.  Thread i packs the codes of 16 consecutive columns of its row
// into one 32-bit word and stores it when column 16 k + 15 or the row's last column is done: word k of row i lies at
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
#include "dtw_parts.h"

static inline int64_t da_ws_bytes(int Fa, int Fb) { return (int64_t)Fa * ag_cdiv(Fb, DTW_PACK) * 4; }

template <bool WALK>
__global__ __launch_bounds__(1024) void dtw_align_kernel(const float* __restrict__ ca, const int32_t* __restrict__ nfa,
                                                         const float* __restrict__ cb, const int32_t* __restrict__ nfb,
                                                         float* __restrict__ total, int32_t* __restrict__ lo,
                                                         int32_t* __restrict__ hi, uint32_t* ws, int Fa, int Fb) {
  __shared__ __attribute__((aligned(16))) float sb[DTW_MAX * DTW_Q];
  __shared__ float edge[2][16];
  __shared__ int32_t slo[DTW_MAX], shi[DTW_MAX];
  const int b = blockIdx.x, i = threadIdx.x;
  const int n = dtw_count(nfa, b, Fa), m = dtw_count(nfb, b, Fb);
  const int W = (Fb + DTW_PACK - 1) / DTW_PACK;
  uint32_t* wsp = ws + (int64_t)b * Fa * W;
  dtw_fill_cols(sb, cb, b, Fb, m, i, blockDim.x);
  float a[DTW_Q];
  dtw_load_row(a, ca, b, Fa, i, n);
  __syncthreads();
  uint32_t word = 0;
  const float cur = dtw_sweep_wg<true>(a, sb, edge, i, n, m, [&](int j, uint32_t dec) {
    word |= dec << (2 * (j & (DTW_PACK - 1)));
    if ((j & (DTW_PACK - 1)) == DTW_PACK - 1 || j == m - 1) {
      wsp[i * W + (j >> 4)] = word;
      word = 0;
    }
  });
  if (i == n - 1) total[b] = cur;
  if (!WALK) return;          // (the profiling tool's forward-only variant; the whole workgroup)

  __threadfence_block();
  __syncthreads();
  if (i == 0) {
    const uint32_t* rd = wsp;
    int ci = n - 1, cj = m - 1, hr = -1, hk = -1;
    uint32_t held = 0;
    shi[cj] = ci;
    for (int t = 0; t < n + m - 2 && (ci | cj) != 0; ++t) {
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
        dec = (held >> (2 * (cj & (DTW_PACK - 1)))) & 3u;
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
  if (Fa < 1 || Fb < 1 || Fa > DTW_MAX || Fb > DTW_MAX) return 0;
  return da_ws_bytes(Fa, Fb);
}

static int da_launch(bool walk, const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b,
                     float* total, int32_t* lo, int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb, void* stream) {
  AG_REQUIRE(cep_a && cep_b && total && lo && hi && ws && B > 0, "ag_dtw_align: bad args");
  AG_REQUIRE(Fa >= 1 && Fb >= 1 && Fa <= DTW_MAX && Fb <= DTW_MAX,
             "ag_dtw_align: sequences of 1 to %d frames (got capacities %d, %d)", DTW_MAX, Fa, Fb);
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

// evalalign.hip -- the two kernels of the aligned distance of the held-out evaluation (audiogan_amd/evaluate.py,
// Evaluator(aligned=True); contracts in include/audiogan_hip.h): per-frame mel cepstra of ragged clips, the DFT as an fp32
// MFMA product, and the dynamic-time-warping total between two batches of cepstral sequences.  Both are fp32 whatever
// ag_set_precision says, use no atomics and add in a fixed order: two runs give the same bits.
#include "common.h"
#include "dtw_parts.h"

// ------------------------------------------------------------------------------------------
// ag_melcep_frames.  Framing, window and the folded transform are those of ag_ltas_power (evalstats.hip):
//     e[0] = f[0],  e[i] = f[i] + f[256 - i] (0 < i < 128),  e[128] = f[128];      o[i] = f[i] - f[256 - i],  o[0] = 0
//     Re X[k] = sum_{i <= 128} e[i] cos(2 pi i k / 256),      -Im X[k] = sum_{1 <= i <= 127} o[i] sin(2 pi i k / 256)
// One workgroup of 4 waves takes (clip, tile of MC_T = 32 frames):
//   1. the tile's span of (32 + 1) * 128 samples goes to LDS once (zeros at and past the clip's length: nothing there is
//      read), with the 256 twiddles ct[m] = cospif(m / 128) and the mel and DCT tables;
//   2. the frames are windowed and folded into two images E [32][131] and O [32][129] - odd pitches, so that the 32 rows of
//      an A fragment fall on 32 different banks (read straight from the raw span, at a pitch of 128 floats, they would
//      all fall on one);
//   3. wave w owns bins 32 w .. 32 w + 31 of all 32 frames: two accumulator tiles of v_mfma_f32_32x32x2_f32, Re = E C
//      (65 steps, k = 0..129, E's column 129 is zero) and Im = O S (64 steps).  Lane l supplies A[frame l & 31][i] and
//      B[i][bin 32 w + (l & 31)], i = i0 + (l >> 5).  B is not a stored matrix: it is ct[(i k) & 255] (cosine) and
//      ct[(i k + 192) & 255] (sine), gathered from the 1 KB table - see DESIGN section 4 for why neither the 132 KB LDS
//      table nor a global one was taken.  Both tiles have the same lane map (bin on the lane, frames in the registers),
//      so re^2 + im^2 is formed in registers and written to a power image P [32][133];
//   4. bin 128 (sum_i (-1)^i e[i]) is a VALU sum: 8 lanes per frame, 17 terms each, then a butterfly;
//   5. power rows go to global memory (optional), the 24 mel sums run over each band's non-zero bins only (their first and
//      last are found once with a ballot: a zero weight adds nothing), E[m] -> logf(E[m] + 1e-10f) into LDS, and 16
//      threads per frame form the 13 cepstra and the 3 zero columns of a 64-byte output row.
// The output is per frame: no workgroup adds to another's, there is no second launch, and a frame's bits do not depend on
// which tile it falls in (every row of an MFMA tile is an independent fma chain in ascending i).
// ------------------------------------------------------------------------------------------
#define MC_N 256
#define MC_HOP 128
#define MC_BINS 129
#define MC_T 32              // frames per workgroup
#define MC_SPAN ((MC_T + 1) * MC_HOP)
#define MC_EP 131            // pitch of E: i = 0..129
#define MC_OP 129            // pitch of O: i = 0..127
#define MC_PP 133            // pitch of P: k = 0..128
#define MC_BANDS 24
#define MC_NCEP 13
#define MC_CEPW 16           // floats per output row
#define MC_LP 25             // pitch of the log-energy image and of the DCT table in LDS

static inline int mc_frames(int n) { return n >= MC_N ? (n - MC_N) / MC_HOP + 1 : 1; }
__device__ __forceinline__ int mc_frames_dev(int n) { return n >= MC_N ? (n - MC_N) / MC_HOP + 1 : 1; }

__global__ __launch_bounds__(256) void melcep_frames_kernel(const float* __restrict__ x, int64_t ldx,
                                                            const int64_t* __restrict__ lens,
                                                            const float* __restrict__ mel, const float* __restrict__ dct,
                                                            float* __restrict__ cep, int32_t* __restrict__ nframes_out,
                                                            float* __restrict__ power, int L, int F) {
  // span (stages 1-2) and P (stages 3-5) share one buffer; so do E (stages 2-4) and the log energies (stage 5)
  __shared__ float sp[MC_T * MC_PP];          // >= MC_SPAN
  __shared__ float se[MC_T * MC_EP];
  __shared__ float so[MC_T * MC_OP];
  __shared__ float ct[MC_N];
  __shared__ float smel[MC_BANDS * MC_BINS];
  __shared__ float sdct[MC_CEPW * MC_LP];
  __shared__ int slo[MC_BANDS], shi[MC_BANDS];
  static_assert(MC_T * MC_PP >= MC_SPAN, "the power image holds the span");
  static_assert(MC_T * MC_EP >= MC_T * MC_LP, "the E image holds the log energies");
  const int b = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  int n;
  {
    const int64_t n64 = lens ? lens[b] : (int64_t)L;
    n = n64 < 0 ? 0 : (n64 > (int64_t)L ? L : (int)n64);
  }
  const int nf = mc_frames_dev(n);
  if (c == 0 && t == 0 && nframes_out) nframes_out[b] = nf;
  const int j0 = c * MC_T;
  if (j0 >= nf) return;          // (the whole workgroup)
  const int nfr = min(MC_T, nf - j0);

  // ---- 1. span, twiddles, tables -----------------------------------------------------------------------------------
  {
    const float* row = x + (int64_t)b * ldx;
    const int t0 = j0 * MC_HOP;
    for (int i = t; i < MC_SPAN; i += 256) sp[i] = (t0 + i < n) ? row[t0 + i] : 0.f;
    ct[t] = cospif((float)t * (1.f / 128.f));
    for (int i = t; i < MC_BANDS * MC_BINS; i += 256) smel[i] = mel[i];
    for (int i = t; i < MC_CEPW * MC_LP; i += 256) {
      const int q = i / MC_LP, m = i - q * MC_LP;
      sdct[i] = (q < MC_NCEP && m < MC_BANDS) ? dct[q * MC_BANDS + m] : 0.f;
    }
  }
  __syncthreads();

  // ---- 2. window and fold; the bands' bin ranges ---------------------------------------------------------------------
  {
    const int i = t & 127;
    const float wi = 0.5f - 0.5f * cospif((float)i * (1.f / 128.f));          // periodic Hann at i (= at 256 - i)
    for (int f = t >> 7; f < MC_T; f += 2) {
      const float a = sp[f * MC_HOP + i];
      const float r = i ? sp[f * MC_HOP + MC_N - i] : 0.f;
      se[f * MC_EP + i] = wi * (a + r);
      so[f * MC_OP + i] = i ? wi * (a - r) : 0.f;
      if (i == 0) {
        se[f * MC_EP + MC_HOP] = sp[f * MC_HOP + MC_HOP];          // w[128] = 1
        se[f * MC_EP + MC_HOP + 1] = 0.f;
      }
    }
    for (int m = w; m < MC_BANDS; m += 4) {          // (wave-uniform)
      const float* r = smel + m * MC_BINS;
      const unsigned long long m0 = __ballot(r[lane] != 0.f), m1 = __ballot(r[64 + lane] != 0.f),
                               m2 = __ballot(lane == 0 && r[128] != 0.f);
      int lo = MC_BINS, hi = -1;
      if (m2) { lo = 128; hi = 128; }
      if (m1) { lo = 64 + __ffsll((long long)m1) - 1; hi = max(hi, 64 + 63 - __clzll((long long)m1)); }
      if (m0) { lo = __ffsll((long long)m0) - 1; hi = max(hi, 63 - __clzll((long long)m0)); }
      if (lane == 0) { slo[m] = lo; shi[m] = hi; }
    }
  }
  __syncthreads();

  // ---- 3. the two products; 4. bin 128 -----------------------------------------------------------------------------------
  {
    const int fr = lane & 31, kh = lane >> 5;
    const int k = 32 * w + fr;          // this lane's bin (B's column)
    f32x16 re, im;
#pragma unroll
    for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
    const float* ea = se + fr * MC_EP + kh;
    const float* oa = so + fr * MC_OP + kh;
    int ci = (kh * k) & (MC_N - 1);          // (i k) mod 256 at i = i0 + kh
    const int st = (2 * k) & (MC_N - 1);
#pragma unroll 4
    for (int i0 = 0; i0 < 128; i0 += 2) {
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[i0], ct[ci], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[i0], ct[(ci + 192) & (MC_N - 1)], im, 0, 0, 0);
      ci = (ci + st) & (MC_N - 1);
    }
    re = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[128], ct[ci], re, 0, 0, 0);          // i = 128 and the zero column 129
    // bin 128 before the span's buffer is reused: it reads E only
    float ny = 0.f;
    {
      const int f = t >> 3, p = t & 7;
      const float* e = se + f * MC_EP;
      for (int i = p; i <= 128; i += 8) ny += (i & 1) ? -e[i] : e[i];
      ny += __shfl_xor(ny, 1, 64);
      ny += __shfl_xor(ny, 2, 64);
      ny += __shfl_xor(ny, 4, 64);
      if (p == 0) sp[f * MC_PP + 128] = ny * ny;          // (the span was consumed before the last barrier)
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = (r & 3) + 8 * (r >> 2) + 4 * kh;
      sp[f * MC_PP + k] = re[r] * re[r] + im[r] * im[r];
    }
  }
  __syncthreads();

  // ---- 5. power rows, mel sums, logarithm, cepstra ---------------------------------------------------------------------------
  if (power) {
    float* dst = power + ((int64_t)b * F + j0) * MC_BINS;
    for (int i = t; i < nfr * MC_BINS; i += 256) {
      const int f = i / MC_BINS, k = i - f * MC_BINS;
      dst[i] = sp[f * MC_PP + k];
    }
  }
  {
    const int f = t & 31;
    const float* p = sp + f * MC_PP;
    for (int m = t >> 5; m < MC_BANDS; m += 8) {
      const float* wr = smel + m * MC_BINS;
      const int hi = shi[m];
      float s = 0.f;
      for (int k = slo[m]; k <= hi; ++k) s = fmaf(wr[k], p[k], s);
      se[f * MC_LP + m] = logf(s + 1e-10f);          // (E was consumed before the last barrier)
    }
  }
  __syncthreads();
  {
    const int q = t & 15;
    const float* dr = sdct + q * MC_LP;
    for (int f = t >> 4; f < nfr; f += 16) {
      const float* lg = se + f * MC_LP;
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < MC_BANDS; ++m) s = fmaf(dr[m], lg[m], s);
      cep[((int64_t)b * F + j0 + f) * MC_CEPW + q] = q < MC_NCEP ? s : 0.f;
    }
  }
}

extern "C" int ag_melcep_frames(const float* x, int64_t ldx, const int64_t* lens_i64, const float* mel, const float* dct,
                                float* cep, int32_t* nframes_out, float* power, int B, int L, void* stream) {
  AG_REQUIRE(x && mel && dct && cep && B > 0 && B <= 65535 && L > 0 && ldx >= L, "ag_melcep_frames: bad args");
  const int F = mc_frames(L);
  const int S = ag_cdiv(F, MC_T);
  AG_REQUIRE(S <= 65535, "ag_melcep_frames: clips of %d samples are too long", L);
  ag_note_kernel("melcep_frames_kernel");
  hipLaunchKernelGGL(melcep_frames_kernel, dim3(B, S), dim3(256), 0, (hipStream_t)stream, x, ldx, lens_i64, mel, dct, cep,
                     nframes_out, power, L, F);
  AG_CHECK_LAUNCH("ag_melcep_frames");
  return AG_OK;
}

// ------------------------------------------------------------------------------------------
// ag_dtw_cost: one workgroup per pair of sequences, rows those of sequence a; the recursion is dtw_parts.h's workgroup sweep.
// Sequence b's LDS is static and sized for the capacity limit, whatever the lengths.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void dtw_cost_kernel(const float* __restrict__ ca, const int32_t* __restrict__ nfa,
                                                        const float* __restrict__ cb, const int32_t* __restrict__ nfb,
                                                        float* __restrict__ out, int Fa, int Fb) {
  __shared__ __attribute__((aligned(16))) float sb[DTW_MAX * DTW_Q];
  __shared__ float edge[2][16];
  const int b = blockIdx.x, i = threadIdx.x;
  const int n = dtw_count(nfa, b, Fa), m = dtw_count(nfb, b, Fb);
  dtw_fill_cols(sb, cb, b, Fb, m, i, blockDim.x);
  float a[DTW_Q];
  dtw_load_row(a, ca, b, Fa, i, n);
  __syncthreads();
  const float cur = dtw_sweep_wg(a, sb, edge, i, n, m);
  if (i == n - 1) out[b] = cur;
}

extern "C" int ag_dtw_cost(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b, float* out,
                           int B, int Fa, int Fb, void* stream) {
  AG_REQUIRE(cep_a && cep_b && out && B > 0 && Fa > 0 && Fb > 0, "ag_dtw_cost: bad args");
  AG_REQUIRE(Fa <= DTW_MAX && Fb <= DTW_MAX, "ag_dtw_cost: sequences of up to %d frames (got capacities %d, %d)", DTW_MAX,
             Fa, Fb);
  ag_note_kernel("dtw_cost_kernel");
  hipLaunchKernelGGL(dtw_cost_kernel, dim3(B), dim3(ag_roundup(Fa, AG_WAVE)), 0, (hipStream_t)stream, cep_a, nf_a, cep_b,
                     nf_b, out, Fa, Fb);
  AG_CHECK_LAUNCH("ag_dtw_cost");
  return AG_OK;
}

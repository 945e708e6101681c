// evalstats.hip -- the two kernels of the held-out evaluation pass (audiogan_amd/evaluate.py; contracts in
// include/audiogan_hip.h): the long-term average power spectrum of ragged clips and the running statistics of a critic
// output.  Both sum in a fixed order (no float atomics): two runs give the same bits.
#include "common.h"

// ------------------------------------------------------------------------------------------
// ag_ltas_power: frames of 256 samples, hop 128, periodic Hann window, 129 bins of a direct 256-point DFT.
//
// The frame is folded before the transform: with f the windowed frame (w[256 - i] = w[i]),
//     e[0] = f[0],  e[i] = f[i] + f[256 - i] (0 < i < 128),  e[128] = f[128];      o[i] = f[i] - f[256 - i],  o[0] = 0
//     Re X[k] = sum_{i <= 128} e[i] cos(2 pi i k / 256),      -Im X[k] = sum_{i < 128} o[i] sin(2 pi i k / 256)
// - half the products of the plain sum.  One workgroup takes LT_CH consecutive frames of one clip, two frames at a time:
// threads 0..127 the even frame of a pair, 128..255 the odd one; thread k of a half owns bin k.  Bin 128 (Nyquist:
// sum_i (-1)^i e[i], real) rides in the imaginary accumulator of bin 0, which is identically zero otherwise: thread 0 feeds
// it e instead of o and reads its "sine" from the cosine table at index 128 i.  So every thread runs the same loop,
//     re += e[i] * ct[(i * k) & 255];   im += (k ? o[i] : e[i]) * ct[(i * km + so) & 255];     (km, so) = (k, 192) or (128, 0)
// (sin(2 pi m / 256) = cos(2 pi (m - 64) / 256); the sign of im is lost in the square).  ct[m] = cospif(m / 128): the
// argument is exact and the function is evaluated, not recurred.  e and o sit in LDS, padded with zeros to 132 entries, and
// are read four at a time, every lane of a wave the same address (a broadcast).
//
// A thread adds re^2 and im^2 of its frames in ascending frame order; the two halves are added even + odd.  A clip with more
// than LT_CH frames is spread over workgroups (grid.y): each writes its partial sums to a slab [B][S][129] and a second
// launch adds them in ascending chunk order and divides by the frame count.  With one chunk the first launch divides itself.
// ------------------------------------------------------------------------------------------
#define LT_N 256
#define LT_HOP 128
#define LT_BINS 129
#define LT_CH 16
#define LT_FOLD 132          // 129 folded samples, padded to whole float4 reads

static inline int lt_frames(int n) { return n >= LT_N ? (n - LT_N) / LT_HOP + 1 : 1; }
__device__ __forceinline__ int lt_frames_dev(int n) { return n >= LT_N ? (n - LT_N) / LT_HOP + 1 : 1; }
__device__ __forceinline__ int lt_len(const int64_t* __restrict__ lens, int b, int L) {
  const int64_t n = lens ? lens[b] : (int64_t)L;
  return n < 0 ? 0 : (n > (int64_t)L ? L : (int)n);
}

__global__ __launch_bounds__(256) void ltas_power_kernel(const float* __restrict__ x, int64_t ldx,
                                                         const int64_t* __restrict__ lens, float* __restrict__ out,
                                                         float* __restrict__ slab, int32_t* __restrict__ nframes_out, int L,
                                                         int S) {
  __shared__ float ct[LT_N];
  __shared__ __attribute__((aligned(16))) float fe[2][LT_FOLD], fo[2][LT_FOLD];
  __shared__ float comb[2][LT_HOP];
  const int b = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const int n = lt_len(lens, b, L);
  const int nf = lt_frames_dev(n);
  if (c == 0 && t == 0 && nframes_out) nframes_out[b] = nf;
  const int j0 = c * LT_CH;
  if (j0 >= nf) return;          // (the whole workgroup: nothing of this chunk exists, the second launch does not read it)
  const int j1 = min(nf, j0 + LT_CH);
  ct[t] = cospif((float)t * (1.f / 128.f));
  const int half = t >> 7, k = t & 127;
  const float w = 0.5f - 0.5f * cospif((float)k * (1.f / 128.f));          // periodic Hann at i = k (= at 256 - k)
  const int km = k ? k : 128, so = k ? 192 : 0;
  const float* row = x + (int64_t)b * ldx;
  if (k < LT_FOLD - LT_HOP) {          // the padding, and o[128] = 0; e[128] is rewritten for every frame
    fe[half][LT_HOP + k] = 0.f;
    fo[half][LT_HOP + k] = 0.f;
  }
  float pa = 0.f, pb = 0.f;
  for (int j = j0; j < j1; j += 2) {
    __syncthreads();          // the table and the padding are written / the previous pair is consumed
    {
      // thread (half, k) folds samples k and 256 - k of frame j + half.  A frame lies inside the clip unless the clip is
      // shorter than one frame: then it is the clip followed by zeros, and nothing at or past n is read
      const int base = (j + half) * LT_HOP;
      const bool live = j + half < j1;
      const float a = (live && base + k < n) ? row[base + k] : 0.f;
      const float r = (live && k > 0 && base + LT_N - k < n) ? row[base + LT_N - k] : 0.f;
      fe[half][k] = w * (a + r);
      fo[half][k] = k ? w * (a - r) : 0.f;
      if (k == 0) fe[half][LT_HOP] = (live && base + LT_HOP < n) ? row[base + LT_HOP] : 0.f;          // w[128] = 1
    }
    __syncthreads();
    if (j + half < j1) {
      const f32x4* e4 = reinterpret_cast<const f32x4*>(fe[half]);
      const f32x4* o4 = reinterpret_cast<const f32x4*>(k ? fo[half] : fe[half]);
      float re = 0.f, im = 0.f;
      int ci = 0, si = so;
      for (int i = 0; i < LT_FOLD / 4; ++i) {
        const f32x4 ve = e4[i], vo = o4[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          re = fmaf(ve[q], ct[ci], re);
          im = fmaf(vo[q], ct[si], im);
          ci = (ci + k) & (LT_N - 1);
          si = (si + km) & (LT_N - 1);
        }
      }
      pa += re * re;
      pb += im * im;
    }
  }
  if (half) {
    comb[0][k] = pa;
    comb[1][k] = pb;
  }
  __syncthreads();
  if (half) return;
  pa += comb[0][k];
  pb += comb[1][k];
  float* dst = S == 1 ? out + (int64_t)b * LT_BINS : slab + ((int64_t)b * S + c) * LT_BINS;
  const float den = S == 1 ? (float)nf : 1.f;
  if (k) {
    dst[k] = (pa + pb) / den;
  } else {
    dst[0] = pa / den;
    dst[LT_HOP] = pb / den;
  }
}

__global__ __launch_bounds__(192) void ltas_finish_kernel(const float* __restrict__ slab, const int64_t* __restrict__ lens,
                                                          float* __restrict__ out, int L, int S) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= LT_BINS) return;
  const int nf = lt_frames_dev(lt_len(lens, b, L));
  const int nc = (nf + LT_CH - 1) / LT_CH;
  const float* p = slab + (int64_t)b * S * LT_BINS + k;
  float s = 0.f;
  for (int c = 0; c < nc; ++c) s += p[(int64_t)c * LT_BINS];
  out[(int64_t)b * LT_BINS + k] = s / (float)nf;
}

static inline int lt_chunks(int L) { return ag_cdiv(lt_frames(L), LT_CH); }

extern "C" int64_t ag_ltas_ws_numel(int B, int L) {
  if (B <= 0 || L <= 0) return 0;
  const int S = lt_chunks(L);
  return S > 1 ? (int64_t)B * S * LT_BINS : 0;
}

extern "C" int ag_ltas_power(const float* x, int64_t ldx, const int64_t* lens_i64, float* out, int32_t* nframes_out, int B,
                             int L, void* stream) {
  const AgWs ws = ag_ws_take();     // FIRST: an argument error below must not leave a stale binding behind
  AG_REQUIRE(x && out && B > 0 && B <= 65535 && L > 0 && ldx >= L, "ag_ltas_power: bad args");
  const int S = lt_chunks(L);
  AG_REQUIRE(S <= 65535, "ag_ltas_power: clips of %d samples are too long", L);
  const int64_t need = ag_ltas_ws_numel(B, L);
  AG_REQUIRE(need == 0 || (ws.p && ws.numel >= need),
             "ag_ltas_power: bind a workspace of >= %lld floats (ag_bind_workspace; ag_ltas_ws_numel)", (long long)need);
  hipStream_t st = (hipStream_t)stream;
  ag_note_kernel("ltas_power_kernel");
  hipLaunchKernelGGL(ltas_power_kernel, dim3(B, S), dim3(256), 0, st, x, ldx, lens_i64, out, need ? ws.p : nullptr,
                     nframes_out, L, S);
  AG_CHECK_LAUNCH("ag_ltas_power");
  if (S > 1) {
    hipLaunchKernelGGL(ltas_finish_kernel, dim3(B), dim3(192), 0, st, ws.p, lens_i64, out, L, S);
    AG_CHECK_LAUNCH("ag_ltas_power(finish)");
  }
  return AG_OK;
}

// ------------------------------------------------------------------------------------------
// ag_score_accum: one workgroup of 16 waves.  Wave w takes rows w, w + 16, ...; inside a row lane l takes t = l, l + 64, ...
// below n_b, so a masked entry is never read.  Per element the loss is fp32 (audiogan.py:191-192, the form of bce_fwd_one_kernel
// in pointwise.hip); every sum is double: the lanes of a wave are added by a butterfly, the 16 waves in wave order.
// Thread 0 then adds the six totals to `acc` with plain loads and stores (launches on one stream are ordered: no atomics).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double es_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(1024) void score_accum_kernel(const float* __restrict__ x, int64_t sxb, int64_t sxt,
                                                           const int64_t* __restrict__ nfr, float target, int positive,
                                                           double* __restrict__ acc, int B, int T) {
  __shared__ double sh[6][16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double clips = 0.0, loss = 0.0, cnt = 0.0, hit = 0.0, sx = 0.0, sxx = 0.0;
  for (int b = wid; b < B; b += 16) {
    const int64_t n64 = nfr ? nfr[b] : (int64_t)T;
    const int n = n64 < 0 ? 0 : (n64 > (int64_t)T ? T : (int)n64);
    if (n < 1) continue;          // (wave-uniform)
    double s = 0.0;
    for (int t = lane; t < n; t += 64) {
      const float v = x[(int64_t)b * sxb + (int64_t)t * sxt];
      const float m = fmaxf(-v, 0.f);
      s += (double)(v - v * target + m + logf(expf(-m) + expf(-v - m)));
      if (positive ? v > 0.f : v < 0.f) hit += 1.0;
      sx += (double)v;
      sxx += (double)v * (double)v;
    }
    loss += es_wave_sum(s) / (double)n;          // (the same value in every lane)
    clips += 1.0;
    cnt += (double)n;
  }
  hit = es_wave_sum(hit);
  sx = es_wave_sum(sx);
  sxx = es_wave_sum(sxx);
  if (lane == 0) {
    sh[0][wid] = clips; sh[1][wid] = loss; sh[2][wid] = cnt; sh[3][wid] = hit; sh[4][wid] = sx; sh[5][wid] = sxx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double r = 0.0;
      for (int w = 0; w < 16; ++w) r += sh[q][w];
      acc[q] += r;
    }
  }
}

extern "C" int ag_score_accum(const float* x, int64_t sxb, int64_t sxt, const int64_t* nframes_i64, float target, int positive,
                              double* acc, int B, int T, void* stream) {
  AG_REQUIRE(x && acc && B > 0 && T > 0 && (int64_t)B * T <= ((int64_t)1 << 22) && (((uintptr_t)acc) & 7) == 0,
             "ag_score_accum: bad args");
  ag_note_kernel("score_accum_kernel");
  hipLaunchKernelGGL(score_accum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, sxb, sxt, nframes_i64, target,
                     positive ? 1 : 0, acc, B, T);
  AG_CHECK_LAUNCH("ag_score_accum");
  return AG_OK;
}

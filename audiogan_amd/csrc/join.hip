// join.hip -- ag_join_facts, ag_join_clips: generated words put next to each other on the device (audiogan_amd/synth.py:
// Voice.say_batch; contract in include/audiogan_hip.h).  The clips are ragged rows whose lengths the generator left on the
// device; the stock form reads every length to the host and adds one slice per word.  Here the plan of a sentence - where
// each word starts, how far neighbours overlap - is computed from those lengths in the prologue of every workgroup, so the
// two launches need no host read.  The reference has no inference path at all (audiogan.py trains and logs).  fp32 whatever
// ag_set_precision says, no atomics, no workspace.
//
// A segment k of a sentence is a window of a row: wave[row * ld + off' .. + n'), off' = clamp(off, 0, L_in), n' = clamp(n, 0,
// L_in - off').  off is arbitrary, so every load of a sample is a 4-byte load.
//
// The arithmetic of an output sample is a product, or the sum of two products, each operation rounded once (the rule's
// fmul_rn / fadd_rn).  A contracted fma would change the bits of about one overlapped sample in four.
#include "common.h"

// __fmul_rn / __fadd_rn are plain * and + inside the HIP headers, compiled there under hipcc's default contraction: once
// inlined, fadd(fmul(a, b), c) becomes one fma.  So the two operations are spelled here, where contraction is off.
#pragma clang fp contract(off)
__device__ __forceinline__ float jn_mul(float a, float b) { return a * b; }          // one product, rounded to nearest even
__device__ __forceinline__ float jn_add(float a, float b) { return a + b; }          // one sum, rounded to nearest even

#define JN_THREADS 256
#define JN_PER 4
#define JN_TILE (JN_THREADS * JN_PER)
#define JN_MAX_SEG 1024          // segments of one sentence: JN_PER per thread in the prologue
#define JN_MAX_FADE 4096

extern "C" int ag_join_max_segments(void) { return JN_MAX_SEG; }

__device__ __forceinline__ void jn_window(int off, int n, int L_in, int& o, int& m) {
  o = off < 0 ? 0 : (off > L_in ? L_in : off);
  const int room = L_in - o;
  m = n < 0 ? 0 : (n > room ? room : n);
}

// ---- ag_join_facts: one workgroup per row ----------------------------------------------------------------------------------
// |x| as bits, as clip_facts_kernel takes it: the largest pattern is the peak, a NaN if there is one, else +inf if there is
// one, else max |x|.
__global__ __launch_bounds__(JN_THREADS) void join_facts_kernel(const float* __restrict__ wave, int64_t ld, int L_in,
                                                                const int32_t* __restrict__ off, const int32_t* __restrict__ n,
                                                                float target, float* __restrict__ gain_out,
                                                                int32_t* __restrict__ bad_out) {
  __shared__ unsigned sh[JN_THREADS / AG_WAVE];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  int o, m;
  jn_window(off[r], n[r], L_in, o, m);
  const unsigned* src = (const unsigned*)(wave + r * ld + o);
  unsigned top = 0;
  for (int t = tid; t < m; t += JN_THREADS) {
    const unsigned a = src[t] & 0x7fffffffu;
    top = a > top ? a : top;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned t2 = (unsigned)__shfl_xor((int)top, s, AG_WAVE);
    top = t2 > top ? t2 : top;
  }
  if ((tid & (AG_WAVE - 1)) == 0) sh[tid / AG_WAVE] = top;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < JN_THREADS / AG_WAVE; ++w) top = sh[w] > top ? sh[w] : top;
    const int bad = top >= 0x7f800000u;
    float g = 1.0f;
    if (bad)
      g = 0.0f;
    else if (target > 0.0f && top > 0)
      g = __fdiv_rn(target, __uint_as_float(top));
    gain_out[r] = g;
    bad_out[r] = bad;
  }
}

extern "C" int ag_join_facts(const float* wave, long long ld, int L_in, const int32_t* off, const int32_t* n, int R, float target,
                             float* gain_out, int32_t* bad_out, void* stream) {
  AG_REQUIRE(R >= 0 && L_in >= 0, "ag_join_facts: %d rows of %d samples: both 0 .. 2^31 - 1", R, L_in);
  if (R == 0) return AG_OK;
  AG_REQUIRE(off && n && gain_out && bad_out && (wave || L_in == 0), "ag_join_facts: null wave, off, n, gain_out or bad_out");
  AG_REQUIRE(ld >= L_in, "ag_join_facts: rows of %d samples at a pitch of %lld", L_in, ld);
  AG_REQUIRE(target == target, "ag_join_facts: the target peak is a NaN");
  ag_note_kernel("join_facts_kernel");
  hipLaunchKernelGGL(join_facts_kernel, dim3((unsigned)R), dim3(JN_THREADS), 0, (hipStream_t)stream, wave, (int64_t)ld, L_in, off,
                     n, target, gain_out, bad_out);
  AG_CHECK_LAUNCH("ag_join_facts");
  return AG_OK;
}

// ---- ag_join_clips: grid (ceil(O_cap / 1024), S) ---------------------------------------------------------------------------
// The prologue, the same in every workgroup of a sentence: thread tid holds segments 4 tid .. 4 tid + 3 of the sentence, their
// windows go to LDS, then their advances adv_k = n_k + pause or n_k - overlap (the overlap needs the neighbour's n: hence
// the barrier), and one exclusive scan of the 1024 advances - four in the thread, a shuffle scan in the wave, the four wave
// totals through LDS - gives the starts.  A segment whose row is outside 0 .. R - 1, and whatever lies past the 1024th
// segment of a sentence, is empty: nothing the tables hold can send a load outside wave.
//
// Then thread tid takes outputs t0 .. t0 + 3, t0 = 1024 blockIdx.x + 4 tid: one binary search for k* = the last k with
// st_k <= t0, a step forward where a later sample passes the next start.  Only k* and k* - 1 can cover a sample (overlaps
// are at most half of either neighbour).  VEC: one 16-byte store; else four 4-byte stores.  The values are the same.
__device__ __forceinline__ float jn_term(const float* __restrict__ wave, int64_t ld, const float* __restrict__ gain,
                                         const float* __restrict__ ramp, int F, int row, int o, int m, int i) {
  const int half = m >> 1, f = F < half ? F : half, j = m - 1 - i;
  float w = 1.0f;
  if (i < f)
    w = ramp[(i * F) / f];
  else if (j < f)
    w = ramp[(j * F) / f];
  const float c = jn_mul(gain[row], w);
  return jn_mul(wave[(int64_t)row * ld + o + i], c);
}

template <int VEC>
__global__ __launch_bounds__(JN_THREADS) void join_clips_kernel(const float* __restrict__ wave, int64_t ld, int L_in,
                                                                const int32_t* __restrict__ off, const int32_t* __restrict__ n,
                                                                const float* __restrict__ gain, int R,
                                                                const int32_t* __restrict__ seg_row,
                                                                const int32_t* __restrict__ join,
                                                                const int32_t* __restrict__ sent_ptr, int K, int pause_max,
                                                                const float* __restrict__ ramp, int F, float* __restrict__ out,
                                                                int64_t ld_out, int O_cap, int64_t* __restrict__ out_len) {
  __shared__ int sh_row[JN_MAX_SEG], sh_off[JN_MAX_SEG], sh_n[JN_MAX_SEG], sh_st[JN_MAX_SEG];
  __shared__ int sh_wave[JN_THREADS / AG_WAVE];
  const int s = blockIdx.y, tid = threadIdx.x;
  int k0 = sent_ptr[s], k1 = sent_ptr[s + 1];
  k0 = k0 < 0 ? 0 : (k0 > K ? K : k0);
  k1 = k1 < k0 ? k0 : (k1 > K ? K : k1);
  const int m = k1 - k0 > JN_MAX_SEG ? JN_MAX_SEG : k1 - k0;
#pragma unroll
  for (int q = 0; q < JN_PER; ++q) {
    const int k = tid * JN_PER + q;
    int row = 0, o = 0, len = 0;
    if (k < m) {
      row = seg_row[k0 + k];
      if (row >= 0 && row < R)
        jn_window(off[row], n[row], L_in, o, len);
      else
        row = 0;
    }
    sh_row[k] = row;
    sh_off[k] = o;
    sh_n[k] = len;
  }
  __syncthreads();
  int adv[JN_PER], mine = 0;
#pragma unroll
  for (int q = 0; q < JN_PER; ++q) {
    const int k = tid * JN_PER + q;
    int a = 0;
    if (k < m) {
      a = sh_n[k];
      if (k + 1 < m) {          // (a sentence's last join is ignored)
        const int jn = join[k0 + k];
        if (jn >= 0) {
          a += jn < pause_max ? jn : pause_max;
        } else {
          const int64_t want = -(int64_t)jn;
          const int ha = sh_n[k] >> 1, hb = sh_n[k + 1] >> 1;
          const int lim = ha < hb ? ha : hb;
          a -= want < lim ? (int)want : lim;
        }
      }
    }
    adv[q] = a;
    mine += a;
  }
  // exclusive scan of the threads' sums: a shuffle scan in the wave, the wave totals through LDS
  const int lane = tid & (AG_WAVE - 1), wid = tid / AG_WAVE;
  int incl = mine;
#pragma unroll
  for (int d = 1; d < AG_WAVE; d <<= 1) {
    const int up = __shfl_up(incl, d, AG_WAVE);
    if (lane >= d) incl += up;
  }
  if (lane == AG_WAVE - 1) sh_wave[wid] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
#pragma unroll
  for (int w = 0; w < JN_THREADS / AG_WAVE; ++w) {
    if (w < wid) base += sh_wave[w];
    total += sh_wave[w];
  }
#pragma unroll
  for (int q = 0; q < JN_PER; ++q) {
    sh_st[tid * JN_PER + q] = base;
    base += adv[q];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) out_len[s] = (int64_t)total;

  const int64_t t0 = (int64_t)blockIdx.x * JN_TILE + tid * JN_PER;          // int64: O_cap may be within 1024 of 2^31
  if (t0 >= O_cap) return;
  // k* = the last k < m with st_k <= t0 (st ascends; -1 for an empty sentence)
  int lo = -1, hi = m;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sh_st[mid] <= t0)
      lo = mid;
    else
      hi = mid;
  }
  int ks = lo;
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < JN_PER; ++q) {
    const int64_t t = t0 + q;
    if (t >= total) break;          // (past the sentence: zeros; total < 2^31)
    while (ks + 1 < m && sh_st[ks + 1] <= t) ++ks;
    const int ib = (int)t - sh_st[ks];
    const bool has_b = ib < sh_n[ks];
    bool has_a = false;
    int ia = 0;
    if (ks > 0) {
      ia = (int)t - sh_st[ks - 1];
      has_a = ia < sh_n[ks - 1];
    }
    float v = 0.f;
    if (has_b) v = jn_term(wave, ld, gain, ramp, F, sh_row[ks], sh_off[ks], sh_n[ks], ib);
    if (has_a) {
      const float va = jn_term(wave, ld, gain, ramp, F, sh_row[ks - 1], sh_off[ks - 1], sh_n[ks - 1], ia);
      v = has_b ? jn_add(va, v) : va;
    }
    y[q] = v;
  }
  float* row_out = out + (int64_t)s * ld_out;
  if (VEC && t0 + JN_PER <= O_cap) {
    *(f32x4*)(row_out + t0) = y;
  } else {
#pragma unroll
    for (int q = 0; q < JN_PER; ++q)
      if (t0 + q < O_cap) row_out[t0 + q] = y[q];
  }
}

extern "C" int ag_join_clips(const float* wave, long long ld, int L_in, const int32_t* off, const int32_t* n, const float* gain,
                             int R, const int32_t* seg_row, const int32_t* join, const int32_t* sent_ptr, int K, int S,
                             int pause_max, const float* ramp, int F, float* out, long long ld_out, int O_cap,
                             long long* out_len, void* stream) {
  AG_REQUIRE(R >= 0 && L_in >= 0 && K >= 0 && O_cap >= 0 && pause_max >= 0,
             "ag_join_clips: R %d, L_in %d, K %d, O_cap %d, pause_max %d: none may be negative", R, L_in, K, O_cap, pause_max);
  AG_REQUIRE(S >= 0 && S <= 65535, "ag_join_clips: %d sentences: 0 .. 65535", S);
  AG_REQUIRE(F >= 0 && F <= JN_MAX_FADE, "ag_join_clips: a fade of %d samples: 0 .. %d", F, JN_MAX_FADE);
  AG_REQUIRE((long long)K <= (long long)S * JN_MAX_SEG,
             "ag_join_clips: %d segments in %d sentences: a sentence holds at most ag_join_max_segments() = %d", K, S, JN_MAX_SEG);
  if (S == 0) return AG_OK;
  {
    const long long most = K < JN_MAX_SEG ? K : JN_MAX_SEG;
    AG_REQUIRE(most * ((long long)L_in + pause_max) <= 0x7fffffffLL,
               "ag_join_clips: %lld segments of up to %d samples with pauses of up to %d: a sentence could pass 2^31 - 1 samples",
               most, L_in, pause_max);
  }
  AG_REQUIRE(sent_ptr && out_len && (out || O_cap == 0), "ag_join_clips: null sent_ptr, out_len or out");
  AG_REQUIRE(K == 0 || (seg_row && join && off && n && gain && (wave || L_in == 0)),
             "ag_join_clips: null wave, off, n, gain, seg_row or join with segments to place");
  AG_REQUIRE(F == 0 || ramp, "ag_join_clips: a fade of %d samples and a null ramp", F);
  AG_REQUIRE(ld >= L_in, "ag_join_clips: source rows of %d samples at a pitch of %lld", L_in, ld);
  AG_REQUIRE(ld_out >= O_cap, "ag_join_clips: rows of %d samples at a pitch of %lld", O_cap, ld_out);
  const int vec = ((uintptr_t)out & 15) == 0 && (ld_out & 3) == 0;
  const dim3 grid((unsigned)(O_cap > 0 ? ag_cdiv64(O_cap, JN_TILE) : 1), (unsigned)S);
  if (vec) {
    ag_note_kernel("join_clips_kernel<1>");
    hipLaunchKernelGGL(join_clips_kernel<1>, grid, dim3(JN_THREADS), 0, (hipStream_t)stream, wave, (int64_t)ld, L_in, off, n, gain,
                       R, seg_row, join, sent_ptr, K, pause_max, ramp, F, out, (int64_t)ld_out, O_cap, (int64_t*)out_len);
  } else {
    ag_note_kernel("join_clips_kernel<0>");
    hipLaunchKernelGGL(join_clips_kernel<0>, grid, dim3(JN_THREADS), 0, (hipStream_t)stream, wave, (int64_t)ld, L_in, off, n, gain,
                       R, seg_row, join, sent_ptr, K, pause_max, ramp, F, out, (int64_t)ld_out, O_cap, (int64_t*)out_len);
  }
  AG_CHECK_LAUNCH("ag_join_clips");
  return AG_OK;
}

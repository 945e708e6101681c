// activity.hip -- ag_frame_power, ag_activity_segments: short-time energy activity detection on the resampled 8 kHz rows
// (audiogan_amd/audio.py: activity, audiogan_amd/ingest.py: build_store(trim / split); contract in include/audiogan_hip.h).
// They stand where the reference's preprocessing cuts words by a forced alignment (preprocess-fisher.py:145-146) or keeps
// the windows whose samples exceed an amplitude threshold (preprocess.py:25-27): an energy gate relative to the loudest
// frame, not an aligner.  fp32 whatever ag_set_precision says, no atomics, no workspace, one launch each.
//
// ---- ag_frame_power: one workgroup of 256 threads per (row, tile of frames) ------------------------------------------------
// With g = gcd(win, hop) every frame starts and ends on a multiple of g of the signal's ABSOLUTE sample index, so the signal
// falls into blocks of g samples that no frame splits.  THE ORDER (the contract's):
//   block sum   S_k = fmaf chain over samples k g .. k g + g - 1, ascending, from a zero accumulator  (s = fmaf(x, x, s))
//   frame       P_f = ((0 + S_{f hq}) + S_{f hq + 1}) + .. + S_{f hq + wq - 1},  hq = hop / g, wq = win / g;  power = P_f * inv_win
// A block sum depends on its g samples alone and a frame on its wq block sums alone - not on the row, the tile, in_start or
// f_start: a signal processed in chunks has the bits of the signal processed at once.  Every sample is loaded once, and
// squared once (it belongs to exactly one block).
//   1. staging: the tile's samples (f0 hop .. (f0 + cnt - 1) hop + win - 1, at most 64 KB with the block sums) go to LDS.
//      Groups of four samples are taken at 16-byte aligned global addresses whatever the row's alignment and the starts
//      (the first group is shifted by m = (address / 4 + first sample) mod 4); a group that lies wholly inside the row's
//      samples is one 16-byte load, one that crosses either end reads its samples one by one, and a sample outside
//      [in_start, in_start + len_b) is a zero that is never loaded.
//   2. block k lies at LDS offset k (g + 1 - g mod 2): an ODD pitch, so the 32 lanes of a ds_read_b32 group, which walk 32
//      blocks in step, are on 32 different banks (at g = 40 an unpadded pitch would put them on 4).  The writes of step 1
//      are ds_write_b32 too: lane l holds samples 4 l .. 4 l + 3, and the four writes go out rotated by l / 8 - in one
//      write lanes l, l + 8, l + 16, l + 24, whose groups start on the same bank, store elements e, e + 1, e + 2, e + 3.
//      The offset's k = j / g is a multiply-high by ceil(2^32 / g), exact for j < 2^20 (a tile holds at most 2^14 samples).
//   3. thread k forms S_k (k, k + 256, ..; the tile is sized so that the blocks fill whole rounds of 256), stored at
//      k + k / 32 when hq is even: frames j, j + 1 read block sums hq apart, and the skew spreads an even stride
//      over the banks (hq = 2: none left; hq odd needs none).
//   4. thread j forms frame j of the tile: wq additions.
// The tile (ag_frame_power_tile) is chosen on the host: among the tiles of up to 256 frames whose samples and block sums fit
// 64 KB, the one with the most frames per round of 256 blocks in step 3 (200 / 80: 126 frames are 255 blocks, one round).
//
// ---- ag_activity_segments: one workgroup of 256 threads per row ------------------------------------------------------------
//   1. all threads: the row's largest power and whether any is not finite.  The maximum is taken on the sign-magnitude
//      bits mapped to ordered integers (-0 below +0): order-free and exact.
//   2. the frames in chunks of 1024: every thread compares four frames with the threshold, a wave's ballot is one 64-bit
//      word of flags in LDS (16 words a chunk), and thread 0 walks the words by count-trailing-zeros from one flip to the
//      next - its work grows with the number of runs, not of frames - while every thread's loads of the next chunk are in
//      flight.  What it carries from chunk to chunk is a handful of registers: the open raw run, the current closed run,
//      the pending sample range and the count; a row of 10^5 frames needs the same 128 bytes of LDS as one of 10.
//      raw run [a, b)   -> joins the current closed run when a - cb < min_gap, else the current one is finished;
//      finished [a, b)  -> dropped when b - a < min_run, else padded to samples and merged into the pending range when it
//                          overlaps or touches it, else the pending range is emitted.
#include "common.h"

#define FP_THREADS 256
#define FP_TILE_MAX 256          // frames: one per thread in step 4
#define FP_LDS_FLOATS 16384      // 64 KB: samples at their padded pitch and the block sums
#define FP_WIN_MAX 4096
#define AS_THREADS 256
#define AS_CHUNK 1024
#define AS_WORDS (AS_CHUNK / 64)
#define AS_UNROLL 8

static inline int fp_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

__host__ __device__ inline int fp_pitch(int g) { return g + 1 - (g & 1); }

// LDS floats of a tile of nb blocks: the samples at the odd pitch, the block sums with their skew
static inline int64_t fp_lds_floats(int64_t nb, int g) { return nb * fp_pitch(g) + nb + (nb >> 5) + 1; }

extern "C" int ag_frame_power_ok(int win, int hop) { return 1 <= hop && hop <= win && win <= FP_WIN_MAX; }

extern "C" int ag_frame_power_tile(int win, int hop) {
  if (!ag_frame_power_ok(win, hop)) return 0;
  const int g = fp_gcd(win, hop), wq = win / g, hq = hop / g;
  int fit = FP_TILE_MAX;
  while (fit > 1 && fp_lds_floats((int64_t)(fit - 1) * hq + wq, g) > FP_LDS_FLOATS) --fit;
  int best = 1, best_rounds = ag_cdiv(wq, FP_THREADS);          // step 3 takes ceil(blocks / 256) rounds
  for (int T = 2; T <= fit; ++T) {
    const int rounds = ag_cdiv((T - 1) * hq + wq, FP_THREADS);
    if ((int64_t)T * best_rounds >= (int64_t)best * rounds) {          // T / rounds >= best / best_rounds
      best = T;
      best_rounds = rounds;
    }
  }
  return best;
}

__global__ __launch_bounds__(FP_THREADS) void frame_power_kernel(const float* __restrict__ src, int64_t src_pitch,
                                                                 const int64_t* __restrict__ src_len, int64_t n_in,
                                                                 int64_t in_start, int win, int hop, int g, unsigned magic,
                                                                 float inv_win, float* __restrict__ dst, int64_t dst_pitch,
                                                                 int64_t f_start, int64_t n_frames, int tile, int tiles,
                                                                 int nbcap) {
  extern __shared__ __attribute__((aligned(16))) float fp_lds[];
  const int pitch = fp_pitch(g);
  const bool padded = pitch != g;
  float* sx = fp_lds;                              // [nbcap][pitch] the samples, block by block
  float* sb = fp_lds + (int64_t)nbcap * pitch;     // the block sums (skewed when hq is even)
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int64_t t0 = (int64_t)(blockIdx.x - b * tiles) * tile;          // first frame of the tile, within the launch
  const int cnt = (int)(n_frames - t0 < (int64_t)tile ? n_frames - t0 : (int64_t)tile);
  const int wq = win / g, hq = hop / g;
  const int nb = (cnt - 1) * hq + wq;          // <= nbcap
  const int S = nb * g;                        // <= 2^14
  const bool skew = !(hq & 1);
  int64_t len = src_len ? src_len[b] : n_in;
  len = len < 0 ? 0 : (len > n_in ? n_in : len);
  const float* row = src + b * src_pitch;
  const int64_t r0 = (f_start + t0) * (int64_t)hop - in_start;          // the tile's first sample, within the row (64 bits)

  // ---- 1. staging ----------------------------------------------------------------------------------------------------
  {
    const int m = (int)((((uintptr_t)row >> 2) + (uint64_t)r0) & 3);          // row + r0 - m is 16-byte aligned
    const int groups = (S + m + 3) >> 2;
    const int rot = (tid >> 3) & 3;
    for (int q = tid; q < groups; q += FP_THREADS) {
      const int j0 = 4 * q - m;                // the group's first sample, within the tile
      const int64_t r = r0 + j0;
      f32x4 v;
      if (r >= 0 && r + 3 < len) {
        v = *(const f32x4*)(row + r);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (r + c >= 0 && r + c < len) ? row[r + c] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int e = (c + rot) & 3;
        const int j = j0 + e;
        const float x = e == 0 ? v[0] : (e == 1 ? v[1] : (e == 2 ? v[2] : v[3]));
        if (j >= 0 && j < S) sx[padded ? j + (int)__umulhi((unsigned)j, magic) : j] = x;
      }
    }
  }
  __syncthreads();

  // ---- 3. block sums ---------------------------------------------------------------------------------------------------
  for (int k = tid; k < nb; k += FP_THREADS) {
    const float* p = sx + k * pitch;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < g; ++i) s = fmaf(p[i], p[i], s);
    sb[skew ? k + (k >> 5) : k] = s;
  }
  __syncthreads();

  // ---- 4. frames -------------------------------------------------------------------------------------------------------
  float* out = dst + b * dst_pitch + t0;
  for (int j = tid; j < cnt; j += FP_THREADS) {
    float acc = 0.f;
    int k = j * hq;
#pragma unroll 4
    for (int i = 0; i < wq; ++i, ++k) acc += sb[skew ? k + (k >> 5) : k];
    out[j] = acc * inv_win;
  }
}

extern "C" int ag_frame_power(const float* src, long long src_pitch, const long long* src_len, long long n_in,
                              long long in_start, int win, int hop, float* dst, long long dst_pitch, long long f_start,
                              long long n_frames, int B, void* stream) {
  AG_REQUIRE(ag_frame_power_ok(win, hop), "ag_frame_power: win %d, hop %d: 1 <= hop <= win <= %d", win, hop, FP_WIN_MAX);
  AG_REQUIRE(B >= 0 && n_in >= 0 && n_frames >= 0 && in_start >= 0 && f_start >= 0 && src_pitch >= 0 && dst_pitch >= 0,
             "ag_frame_power: a negative size or start");
  if (B == 0 || n_frames == 0) return AG_OK;
  AG_REQUIRE(dst && (src || n_in == 0), "ag_frame_power: null src or dst");
  AG_REQUIRE(((uintptr_t)src & 3) == 0, "ag_frame_power: src must be 4-byte aligned");
  AG_REQUIRE(n_in <= (1LL << 56) && src_pitch >= n_in && dst_pitch >= n_frames,
             "ag_frame_power: rows of %lld samples at a pitch of %lld, %lld frames at a pitch of %lld", n_in, src_pitch,
             n_frames, dst_pitch);
  AG_REQUIRE(f_start <= (1LL << 40) && n_frames <= (1LL << 40) && in_start <= (1LL << 60),
             "ag_frame_power: f_start %lld, n_frames %lld: at most 2^40", f_start, n_frames);
  const int tile = ag_frame_power_tile(win, hop);
  const int64_t tiles = ag_cdiv64(n_frames, tile);
  AG_REQUIRE(tiles * B <= 0x7fffffffLL, "ag_frame_power: %lld tiles of %d frames in %d rows: too many for one launch",
             (long long)tiles, tile, B);
  const int g = fp_gcd(win, hop);
  const int nbcap = (tile - 1) * (hop / g) + win / g;
  const size_t lds = (size_t)fp_lds_floats(nbcap, g) * sizeof(float);          // <= 64 KB by the tile's choice
  const unsigned magic = (unsigned)(((1ULL << 32) + (unsigned)g - 1) / (unsigned)g);          // (used for even g only: < 2^32)
  ag_note_kernel("frame_power_kernel");
  hipLaunchKernelGGL(frame_power_kernel, dim3((unsigned)(tiles * B)), dim3(FP_THREADS), lds, (hipStream_t)stream, src,
                     (int64_t)src_pitch, (const int64_t*)src_len, (int64_t)n_in, (int64_t)in_start, win, hop, g, magic,
                     1.0f / (float)win, dst, (int64_t)dst_pitch, (int64_t)f_start, (int64_t)n_frames, tile, (int)tiles, nbcap);
  AG_CHECK_LAUNCH("ag_frame_power");
  return AG_OK;
}

// ---- ag_activity_segments ------------------------------------------------------------------------------------------------
// fp32 bits -> integers in the order of the values (-0 below +0); its own inverse
__device__ __forceinline__ int as_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

extern "C" int ag_activity_chunk(void) { return AS_CHUNK; }

__global__ __launch_bounds__(AS_THREADS) void activity_segments_kernel(const float* __restrict__ power, int64_t power_pitch,
                                                                       const int32_t* __restrict__ nf, int F,
                                                                       const int64_t* __restrict__ len, float ratio, float floor_,
                                                                       int min_gap, int min_run, int pad, int win, int hop,
                                                                       int64_t* __restrict__ seg, int K,
                                                                       int32_t* __restrict__ count_out,
                                                                       float* __restrict__ pmax_out) {
  __shared__ unsigned long long words[AS_WORDS];
  __shared__ int red[2 * (AS_THREADS / AG_WAVE)];
  const int tid = threadIdx.x, lane = tid & (AG_WAVE - 1), wid = tid / AG_WAVE;
  const int64_t b = blockIdx.x;
  int nfb = nf[b];
  nfb = nfb < 0 ? 0 : (nfb > F ? F : nfb);
  int64_t lenb = len[b];
  lenb = lenb < 0 ? 0 : lenb;
  const float* row = power + b * power_pitch;

  // ---- 1. the largest power; any NaN or infinity ---------------------------------------------------------------------
  int key = (int)0x80000000, bad = 0;
  for (int64_t f0 = tid; f0 < nfb; f0 += AS_UNROLL * AS_THREADS) {          // AS_UNROLL independent loads in flight per thread
    int bits[AS_UNROLL];          // (frame indices in 64 bits: F may be within a chunk of 2^31)
#pragma unroll
    for (int u = 0; u < AS_UNROLL; ++u) bits[u] = f0 + u * AS_THREADS < nfb ? __float_as_int(row[f0 + u * AS_THREADS]) : 0;
#pragma unroll
    for (int u = 0; u < AS_UNROLL; ++u) {
      bad |= (bits[u] & 0x7f800000) == 0x7f800000;
      const int k = f0 + u * AS_THREADS < nfb ? as_key(bits[u]) : (int)0x80000000;
      key = k > key ? k : key;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int k2 = __shfl_xor(key, o, AG_WAVE);
    key = k2 > key ? k2 : key;
    bad |= __shfl_xor(bad, o, AG_WAVE);
  }
  if (lane == 0) {
    red[2 * wid] = key;
    red[2 * wid + 1] = bad;
  }
  __syncthreads();
  for (int w = 0; w < AS_THREADS / AG_WAVE; ++w) {
    key = red[2 * w] > key ? red[2 * w] : key;
    bad |= red[2 * w + 1];
  }
  if (bad || nfb == 0) {          // (workgroup-uniform)
    if (tid == 0) {
      count_out[b] = bad ? -1 : 0;
      pmax_out[b] = bad ? __int_as_float(0x7fc00000) : 0.f;
    }
    return;
  }
  const float pmax = __int_as_float(as_key(key));
  const float thr = fmaxf(pmax * ratio, floor_);

  // ---- 2. the runs -------------------------------------------------------------------------------------------------------
  // thread 0's state (the other threads carry copies they never use)
  int in_run = 0, ra = 0;                      // an open raw run and its first frame
  int have_cur = 0, ca = 0, cb = 0;            // the current closed run [ca, cb)
  int have_pend = 0, count = 0;                // the pending sample range [ps, pe)
  int64_t ps = 0, pe = 0;
  int64_t* out = seg + b * (int64_t)K * 2;
  auto flush = [&]() {
    if (count < K) {
      out[2 * (int64_t)count] = ps;
      out[2 * (int64_t)count + 1] = pe;
    }
    ++count;
  };
  auto finished = [&](int a, int e) {
    if (e - a < min_run) return;
    int64_t s0 = ((int64_t)a - pad) * hop, s1 = ((int64_t)e - 1 + pad) * hop + win;
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > lenb ? lenb : s1;
    if (have_pend && s0 <= pe) {
      pe = s1 > pe ? s1 : pe;
    } else {
      if (have_pend) flush();
      ps = s0;
      pe = s1;
      have_pend = 1;
    }
  };
  auto raw = [&](int a, int e) {
    if (have_cur && a - cb < min_gap) {
      cb = e;
    } else {
      if (have_cur) finished(ca, cb);
      ca = a;
      cb = e;
      have_cur = 1;
    }
  };
  float nxt[AS_CHUNK / AS_THREADS];          // the next chunk's powers, loaded while thread 0 walks this one's flags
#pragma unroll
  for (int i = 0; i < AS_CHUNK / AS_THREADS; ++i) {
    const int f = i * AS_THREADS + tid;
    nxt[i] = f < nfb ? row[f] : 0.f;
  }
  for (int64_t c0 = 0; c0 < nfb; c0 += AS_CHUNK) {
#pragma unroll
    for (int i = 0; i < AS_CHUNK / AS_THREADS; ++i) {
      const bool act = c0 + i * AS_THREADS + tid < nfb && nxt[i] > thr;
      const unsigned long long mask = __ballot(act);
      if (lane == 0) words[i * (AS_THREADS / AG_WAVE) + wid] = mask;
    }
#pragma unroll
    for (int i = 0; i < AS_CHUNK / AS_THREADS; ++i) {
      const int64_t f = c0 + AS_CHUNK + i * AS_THREADS + tid;
      nxt[i] = f < nfb ? row[f] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long wd[AS_WORDS];
#pragma unroll
      for (int w = 0; w < AS_WORDS; ++w) wd[w] = words[w];
#pragma unroll
      for (int w = 0; w < AS_WORDS; ++w) {
        unsigned long long bits = wd[w];
        const int64_t base = c0 + w * 64;
        for (;;) {
          if (!in_run) {
            if (!bits) break;
            const int t = __builtin_ctzll(bits);
            ra = (int)(base + t);
            in_run = 1;
            bits |= (1ull << t) - 1;          // look for the next clear bit
          }
          const unsigned long long clear = ~bits;
          if (!clear) break;                  // the run goes on into the next word
          const int t = __builtin_ctzll(clear);
          raw(ra, (int)(base + t));
          in_run = 0;
          bits &= ~((1ull << t) - 1);         // (bit t is clear already)
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (in_run) raw(ra, nfb);
    if (have_cur) finished(ca, cb);
    if (have_pend) flush();
    count_out[b] = count;
    pmax_out[b] = pmax;
  }
}

extern "C" int ag_activity_segments(const float* power, long long power_pitch, const int32_t* nf, int F, const long long* len,
                                    float ratio, float floor_, int min_gap, int min_run, int pad, int win, int hop,
                                    long long* seg, int K, int32_t* count, float* pmax, int B, void* stream) {
  AG_REQUIRE(min_gap >= 0 && min_run >= 0 && pad >= 0 && K >= 0 && F >= 0,
             "ag_activity_segments: min_gap %d, min_run %d, pad %d, K %d, F %d: none may be negative", min_gap, min_run, pad, K, F);
  AG_REQUIRE(B >= 0 && B <= 65535, "ag_activity_segments: B %d: 0 .. 65535", B);
  AG_REQUIRE(ag_frame_power_ok(win, hop), "ag_activity_segments: win %d, hop %d: 1 <= hop <= win <= %d", win, hop, FP_WIN_MAX);
  if (B == 0) return AG_OK;
  AG_REQUIRE(power_pitch >= F, "ag_activity_segments: rows of %d frames at a pitch of %lld", F, power_pitch);
  AG_REQUIRE((power || F == 0) && nf && len && count && pmax && (seg || K == 0),
             "ag_activity_segments: null power, nf, len, seg, count or pmax");
  ag_note_kernel("activity_segments_kernel");
  hipLaunchKernelGGL(activity_segments_kernel, dim3((unsigned)B), dim3(AS_THREADS), 0, (hipStream_t)stream, power,
                     (int64_t)power_pitch, nf, F, (const int64_t*)len, ratio, floor_, min_gap, min_run, pad, win, hop,
                     (int64_t*)seg, K, count, pmax);
  AG_CHECK_LAUNCH("ag_activity_segments");
  return AG_OK;
}

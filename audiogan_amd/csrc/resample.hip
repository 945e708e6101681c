// resample.hip -- ag_resample_poly: polyphase windowed-sinc resampling of ragged rows of interleaved PCM frames to the
// models' rate (audiogan_amd/audio.py: resample, audiogan_amd/ingest.py: build_store; contract in include/audiogan_hip.h).
// It stands where the reference's preprocessing calls librosa.load(wav, sr=8000) (preprocess.py:24,
// preprocess-fisher.py:232).  fp32 whatever ag_set_precision says, no atomics, no workspace, one launch.
//
// Output N of a row is  y[N] = sum_{t < taps} bank[p, t] x[base - half + t],  base = (N M) div L,  p = (N M) mod L,
// half = (taps - 1) / 2, N M formed in 64 bits.  One workgroup of 256 threads takes (row, tile of `tile` outputs):
//   1. the tile's input window - frames base(N0) - half .. base(N0 + cnt - 1) + half, at most ceil((tile - 1) M / L) + 1 +
//      taps of them - is converted and downmixed ONCE into LDS; a frame outside [in_start, in_start + len_b) is a zero that
//      is never loaded;
//   2. the bank [L, taps] goes to LDS beside it at a row pitch of `taps` floats.  taps is odd (the launcher insists), so
//      an odd pitch needs no padding: lanes n, n + 1 read phase rows p, p + (M mod L), and with an odd pitch rows that
//      differ mod 32 start on different banks of the 32 a ds_read_b32 lane group sees.  L = 1 is one row that every lane
//      reads at one address (a broadcast);
//   3. thread i forms outputs i, i + 256, .. of the tile (four of a tile of 1024, two of 512, else one), each an fmaf
//      chain over t = 0 .. taps - 1 from a zero accumulator.  That chain is the whole of an output's arithmetic: it
//      depends on the source values and the phase row alone, not on n, b, out_start or the tile - a signal resampled in
//      chunks has the bits of the same signal resampled at once.  When L divides 256 the outputs of a thread share their
//      phase, and a coefficient is read once for all of them (5 LDS reads per 4 fmaf instead of 8); the chains are the
//      same either way.  Within a tile the indices are 32-bit: the launcher refuses M above 2^20.
// The tile is chosen on the host: the largest power of two up to 1024 whose window and bank fit 80 KB of LDS (two
// workgroups on a CU's 160 KB), else the largest that fits 160 KB - which a bank the predicate admits (L taps 4 <= 64 KB)
// always allows: at a tile of one output the window is taps + 2 floats.
#include "common.h"

#define RS_THREADS 256
#define RS_PER 4
#define RS_TILE (RS_THREADS * RS_PER)
#define RS_LDS_SHARED (80 * 1024)
#define RS_LDS_MAX (160 * 1024)
#define RS_BANK_MAX 65536
#define RS_M_MAX (1 << 20)          // a tile's index arithmetic stays in 32 bits

// the mono sample of frame r of a row: channels added in order in fp32, times 1 / C; int16 then scaled by 2^-15
__device__ __forceinline__ float rs_mono(const void* __restrict__ row, int kind, int C, float invc, int64_t r) {
  float s;
  if (kind == 0) {
    const float* f = (const float*)row + r * C;
    s = f[0];
    for (int c = 1; c < C; ++c) s += f[c];
    s *= invc;
  } else {
    const int16_t* f = (const int16_t*)row + r * C;
    s = (float)f[0];
    for (int c = 1; c < C; ++c) s += (float)f[c];
    s *= invc;
    s *= (1.0f / 32768.0f);
  }
  return s;
}

// outputs tid, tid + 256, .. (PER of them) of a tile: each one fmaf chain over t ascending from a zero accumulator.  SAME: L
// divides 256, so the thread's outputs share their phase row and a coefficient is read once for PER fmaf.
template <int PER, bool SAME>
__device__ __forceinline__ void rs_outputs(const float* sx, const float* sb, float* __restrict__ out, int tid, int cnt, int p0,
                                           int L, int M, int taps) {
  const float* xr[PER];
  const float* cr[PER];
  float acc[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = tid + RS_THREADS * k;
    int o = 0, p = 0;
    if (j < cnt) {          // (an idle slot reads the window's first taps and stores nothing)
      const unsigned rel = (unsigned)p0 + (unsigned)j * (unsigned)M;          // < L + 1024 M < 2^31: M <= RS_M_MAX
      o = (int)(rel / (unsigned)L);
      p = (int)(rel - (unsigned)o * (unsigned)L);
    }
    xr[k] = sx + o;
    cr[k] = sb + p * taps;
    acc[k] = 0.f;
  }
#pragma unroll 4
  for (int t = 0; t < taps; ++t) {
    if (SAME) {
      const float c = cr[0][t];
#pragma unroll
      for (int k = 0; k < PER; ++k) acc[k] = fmaf(c, xr[k][t], acc[k]);
    } else {
#pragma unroll
      for (int k = 0; k < PER; ++k) acc[k] = fmaf(cr[k][t], xr[k][t], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = tid + RS_THREADS * k;
    if (j < cnt) out[j] = acc[k];
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(
    const void* __restrict__ src, int kind, int C, int64_t src_pitch, const int64_t* __restrict__ src_len, int64_t n_in,
    int64_t in_start, const float* __restrict__ bank, int L, int M, int taps, float* __restrict__ dst, int64_t dst_pitch,
    int64_t n_out, int64_t out_start, int tile, int tiles, int wcap) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  float* sx = rs_lds;                // [wcap] the window
  float* sb = rs_lds + wcap;         // [L][taps] the bank
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int64_t n0 = (int64_t)(blockIdx.x - b * tiles) * tile;          // first output of the tile, within the row
  const int cnt = (int)(n_out - n0 < (int64_t)tile ? n_out - n0 : (int64_t)tile);
  const int half = (taps - 1) >> 1;
  const int64_t q0 = (out_start + n0) * (int64_t)M;          // 64 bits: out_start may be past 2^31
  const int64_t base0 = q0 / L;
  const int p0 = (int)(q0 - base0 * L);
  const int wlen = (int)(((int64_t)p0 + (int64_t)(cnt - 1) * M) / L) + taps;          // <= wcap
  int64_t len = src_len ? src_len[b] : n_in;
  len = len < 0 ? 0 : (len > n_in ? n_in : len);

  // ---- 1. window, 2. bank ----------------------------------------------------------------------------------------
  {
    const void* row = kind == 0 ? (const void*)((const float*)src + b * src_pitch)
                                : (const void*)((const int16_t*)src + b * src_pitch);
    const float invc = 1.0f / (float)C;
    const int64_t r0 = base0 - half - in_start;          // the window's first frame, within the row
    for (int i = tid; i < wlen; i += RS_THREADS) {
      const int64_t r = r0 + i;
      sx[i] = (r >= 0 && r < len) ? rs_mono(row, kind, C, invc, r) : 0.f;
    }
    const int nb = L * taps;
    for (int i = tid; i < nb; i += RS_THREADS) sb[i] = bank[i];
  }
  __syncthreads();

  // ---- 3. the outputs --------------------------------------------------------------------------------------------
  float* out = dst + b * dst_pitch + n0;
  const bool same = (RS_THREADS % L) == 0;          // (workgroup-uniform) one phase per thread
  if (tile > 2 * RS_THREADS) {
    if (same) rs_outputs<4, true>(sx, sb, out, tid, cnt, p0, L, M, taps);
    else rs_outputs<4, false>(sx, sb, out, tid, cnt, p0, L, M, taps);
  } else if (tile > RS_THREADS) {
    if (same) rs_outputs<2, true>(sx, sb, out, tid, cnt, p0, L, M, taps);
    else rs_outputs<2, false>(sx, sb, out, tid, cnt, p0, L, M, taps);
  } else {
    rs_outputs<1, false>(sx, sb, out, tid, cnt, p0, L, M, taps);
  }
}

extern "C" int ag_resample_ok(int L, int M, int taps, int channels, int src_kind) {
  if (L < 1 || M < 1 || taps < 3 || !(taps & 1)) return 0;
  if ((int64_t)L * taps * 4 > RS_BANK_MAX) return 0;
  if (channels < 1 || channels > 8) return 0;
  return src_kind == 0 || src_kind == 1;
}

// floats of the window of a tile of `tile` outputs (an upper bound of the kernel's wlen)
static inline int64_t rs_window(int tile, int L, int M, int taps) {
  return ((int64_t)(tile - 1) * M + L - 1) / L + 1 + taps;
}

extern "C" int ag_resample_poly(const void* src, int src_kind, int channels, long long src_pitch, const long long* src_len,
                                long long n_in, long long in_start, const float* bank, int L, int M, int taps, float* dst,
                                long long dst_pitch, long long n_out, long long out_start, int B, void* stream) {
  AG_REQUIRE(ag_resample_ok(L, M, taps, channels, src_kind),
             "ag_resample_poly: L %d, M %d, taps %d, %d channels, kind %d: L, M >= 1, taps odd and >= 3, L taps 4 <= %d bytes, "
             "1..8 channels, kind 0 (fp32) or 1 (int16)", L, M, taps, channels, src_kind, RS_BANK_MAX);
  AG_REQUIRE(M <= RS_M_MAX, "ag_resample_poly: M %d: at most %d", M, RS_M_MAX);
  AG_REQUIRE(B >= 0 && n_in >= 0 && n_out >= 0 && in_start >= 0 && out_start >= 0 && src_pitch >= 0 && dst_pitch >= 0,
             "ag_resample_poly: a negative size");
  if (B == 0 || n_out == 0) return AG_OK;
  AG_REQUIRE(src && dst && bank, "ag_resample_poly: null src, dst or bank");
  AG_REQUIRE(n_in <= (1LL << 56) && src_pitch >= n_in * channels && dst_pitch >= n_out,
             "ag_resample_poly: rows of %lld frames of %d channels at a pitch of %lld, %lld outputs at a pitch of %lld", n_in,
             channels, src_pitch, n_out, dst_pitch);
  AG_REQUIRE(out_start <= (1LL << 40) && n_out <= (1LL << 40) && in_start <= (1LL << 60),
             "ag_resample_poly: out_start %lld, n_out %lld: at most 2^40", out_start, n_out);
  int tile = 0;
  for (const int64_t cap : {(int64_t)RS_LDS_SHARED, (int64_t)RS_LDS_MAX}) {
    for (int t = RS_TILE; t >= 1 && !tile; t >>= 1)
      if ((rs_window(t, L, M, taps) + (int64_t)L * taps) * 4 <= cap) tile = t;
    if (tile) break;
  }
  AG_REQUIRE(tile > 0, "ag_resample_poly: no tile of L %d, M %d, taps %d fits the LDS", L, M, taps);
  const int64_t tiles = ag_cdiv64(n_out, tile);
  AG_REQUIRE(tiles * B <= 0x7fffffffLL, "ag_resample_poly: %lld tiles of %d outputs in %d rows: too many for one launch",
             (long long)tiles, tile, B);
  const int wcap = (int)rs_window(tile, L, M, taps);
  const size_t lds = ((size_t)wcap + (size_t)L * taps) * sizeof(float);
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)resample_poly_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess) {
    ag_set_error("ag_resample_poly: %zu bytes of LDS refused", lds);
    return AG_ERR_LAUNCH;
  }
  ag_note_kernel("resample_poly_kernel");
  hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), lds, (hipStream_t)stream, src,
                     src_kind, channels, (int64_t)src_pitch, (const int64_t*)src_len, (int64_t)n_in, (int64_t)in_start, bank,
                     L, M, taps, dst, (int64_t)dst_pitch, (int64_t)n_out, (int64_t)out_start, tile, (int)tiles, wcap);
  AG_CHECK_LAUNCH("ag_resample_poly");
  return AG_OK;
}

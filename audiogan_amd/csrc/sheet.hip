// sheet.hip -- ag_sheet_render: a minibatch of ragged clips drawn as ONE contact sheet, uint8 [H, W, 3], in one launch
// (audiogan_amd/sheet.py: render, SheetWriter; contract in include/audiogan_hip.h).  The reference plots every sample's waveform
// on the host (audiogan.py:639-653); here the clips' lengths, peaks and spectral maxima stay on the device - every workgroup
// redoes its clip's two maxima in its prologue, as ag_join_clips redoes its plan - so a sample step between two graph replays
// reads nothing back.  fp32 whatever ag_set_precision says, no atomics, no workspace, no logarithm: the level of a
// spectrogram cell is a binary search of P against thresholds[l] * Pmax.
//
// A workgroup owns columns j0 .. j0 + 31 of one grid cell over the cell's whole height, with the gutter below it, the gutter to
// its right if it holds the cell's last column, and the sheet's top / left gutter if the cell is in the first row / column:
// the rectangles tile the image, so every pixel is written exactly once.  Pixels are 3 bytes at any alignment: a chunk of 32
// pixel rows is formed in LDS at the byte phase its row has in memory, then stored as whole dwords, with single bytes only at
// a row segment's two ragged ends.
#include "common.h"

// (the envelope's row is a stated chain of single roundings: no contraction)
#pragma clang fp contract(off)

#define SH_THREADS 256
#define SH_TC 32                       // tile columns (hops) per workgroup
#define SH_BINS 129
#define SH_MAX_GUTTER 16
#define SH_XW (SH_TC + 2 * SH_MAX_GUTTER)          // the widest rectangle, in pixels: 64
#define SH_RC 32                       // pixel rows formed at a time
#define SH_PITCH 49                    // dwords of a staged row: 3 * 64 bytes + a phase of up to 3, rounded up
#define SH_MAX_STRIP 4096
#define SH_ILP 8                        // loads of each array in flight per thread in the prologue

extern "C" int ag_sheet_tile_columns(void) { return SH_TC; }

// max over the workgroup of values >= 0; fmaxf drops a NaN, so the result does not depend on the order
__device__ __forceinline__ float sh_block_max(float v, float* sh) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, AG_WAVE));
  __syncthreads();
  if ((threadIdx.x & (AG_WAVE - 1)) == 0) sh[threadIdx.x / AG_WAVE] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < SH_THREADS / AG_WAVE; ++w) r = fmaxf(r, sh[w]);
  return r;
}

// the row of the strip a sample value lands on: row 0 is +peak, row Hw - 1 is -peak.  half = 0.5f * (Hw - 1), top = Hw - 1.
__device__ __forceinline__ int sh_row(float v, float peak, float half, float top) {
  const float u = __fdiv_rn(v, peak);
  const float d = 1.0f - u;
  float y = d * half;
  y = fminf(fmaxf(y, 0.0f), top);          // (a NaN - inf / inf - becomes row 0)
  return (int)rintf(y);
}

__global__ __launch_bounds__(SH_THREADS) void sheet_render_kernel(
    const float* __restrict__ wave, int64_t ld, const int64_t* __restrict__ lens, int L, const float* __restrict__ power,
    const int32_t* __restrict__ nframes, int F, int B, const float* __restrict__ thresholds,
    const unsigned char* __restrict__ cmap, uint32_t bg, uint32_t paper, uint32_t ink, int cols, int Hw, int gutter,
    unsigned char* __restrict__ img, int W) {
  __shared__ float sh_pow[SH_TC * SH_BINS];
  __shared__ float sh_thr[256];
  __shared__ uint32_t sh_cmap[256];
  __shared__ int sh_r0[SH_TC], sh_r1[SH_TC];
  __shared__ uint32_t sh_pix[SH_RC * SH_PITCH];
  __shared__ float sh_red[SH_THREADS / AG_WAVE];
  const int tid = threadIdx.x, lane = tid & (AG_WAVE - 1), wid = tid / AG_WAVE;
  const int cell = blockIdx.y, ct = blockIdx.x;
  const int r = cell / cols, q = cell - r * cols;
  const int Wt = (L + 127) >> 7, Ht = Hw + SH_BINS;
  const int x0 = gutter + q * (Wt + gutter), y0 = gutter + r * (Ht + gutter);
  const int j0 = ct * SH_TC;
  const int jw = Wt - j0 < SH_TC ? Wt - j0 : SH_TC;
  // the rectangle [xs, xe) x [ys, ye)
  int xs = x0 + j0, xe = xs + jw;
  if (ct == (int)gridDim.x - 1) xe += gutter;
  if (ct == 0 && q == 0) xs = 0;
  const int ys = r == 0 ? 0 : y0, ye = y0 + Ht + gutter;

  sh_thr[tid] = thresholds[tid];
  sh_cmap[tid] = (uint32_t)cmap[3 * tid] | ((uint32_t)cmap[3 * tid + 1] << 8) | ((uint32_t)cmap[3 * tid + 2] << 16);

  const bool live = cell < B;          // (uniform over the workgroup; an unused grid cell is all background)
  int n = 0, nf = 0, ncol = 0;
  float pmax = 0.0f;
  if (live) {
    if (lens) {
      const int64_t v = lens[cell];
      n = v < 0 ? 0 : (v > L ? L : (int)v);
    } else {
      n = L;
    }
    const int fcap = F < Wt ? F : Wt;
    nf = nframes[cell];
    nf = nf < 0 ? 0 : (nf > fcap ? fcap : nf);
    ncol = (n + 127) >> 7;
    const float* w = wave + (int64_t)cell * ld;
    const float* pw = power + (int64_t)cell * F * SH_BINS;
    float peak = 0.0f;
    // (both maxima in one loop, eight loads of each in flight per thread: the prologue is latency, not bandwidth)
    const int np = nf * SH_BINS;
    const int most = n > np ? n : np;
    for (int i = tid; i < most; i += SH_ILP * SH_THREADS) {
      float a[SH_ILP], p[SH_ILP];
#pragma unroll
      for (int q = 0; q < SH_ILP; ++q) {
        const int k = i + q * SH_THREADS;
        a[q] = k < n ? fabsf(w[k]) : 0.0f;
        p[q] = k < np ? pw[k] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < SH_ILP; ++q) {
        peak = fmaxf(peak, a[q]);
        pmax = fmaxf(pmax, p[q]);
      }
    }
    peak = sh_block_max(peak, sh_red);
    pmax = sh_block_max(pmax, sh_red);
    // this tile's frames, as they lie in memory: [frame][bin], read back along the frames at the odd pitch 129
    const int jn = (j0 + jw < nf ? j0 + jw : nf) - j0;
#pragma unroll 8
    for (int i = tid; i < jn * SH_BINS; i += SH_THREADS) sh_pow[i] = pw[(int64_t)j0 * SH_BINS + i];
    // the envelope of this tile's columns: one wave per column, two samples per lane
    const float half = 0.5f * (float)(Hw - 1), top = (float)(Hw - 1);
    for (int c = wid; c < jw; c += SH_THREADS / AG_WAVE) {
      const int j = j0 + c;
      if (j >= ncol) break;
      const int t0 = j * 128 + lane, t1 = t0 + 64;
      float lo = INFINITY, hi = -INFINITY;
      if (t0 < n) {
        const float v = w[t0];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
      if (t1 < n) {
        const float v = w[t1];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, s, AG_WAVE));
        hi = fmaxf(hi, __shfl_xor(hi, s, AG_WAVE));
      }
      if (lane == 0) {
        int a = (Hw - 1) >> 1, b = a;          // a silent clip: the centre line
        if (peak > 0.0f) {
          if (!(lo <= hi)) lo = hi = 0.0f;          // (every sample of the column a NaN)
          a = sh_row(hi, peak, half, top);
          b = sh_row(lo, peak, half, top);
        }
        sh_r0[c] = a < b ? a : b;
        sh_r1[c] = a < b ? b : a;
      }
    }
  }
  __syncthreads();

  const int rw = xe - xs;          // <= SH_XW
  const int px = tid & (SH_XW - 1), pr = tid / SH_XW;
  const uintptr_t base = (uintptr_t)img;
  for (int yc = ys; yc < ye; yc += SH_RC) {
#pragma unroll
    for (int rr = pr; rr < SH_RC; rr += SH_THREADS / SH_XW) {          // (unrolled: eight searches in flight per thread)
      const int y = yc + rr;
      if (y < ye && px < rw) {
        const int x = xs + px, ty = y - y0, tx = x - x0;
        uint32_t col = bg;
        if (live && ty >= 0 && ty < Ht && tx >= 0 && tx < Wt) {
          const int c = tx - j0;
          if (ty < Hw) {
            if (tx < ncol) col = (ty >= sh_r0[c] && ty <= sh_r1[c]) ? ink : paper;
          } else if (tx < nf) {
            const float P = sh_pow[c * SH_BINS + (SH_BINS - 1 - (ty - Hw))];
            // the largest l in 1 .. 255 with P >= thresholds[l] * Pmax, 0 if there is none (level 0 either way at l = 0): the
            // table ascends, so eight halving steps find it
            int lvl = 0;
            if (pmax > 0.0f) {
#pragma unroll
              for (int step = 128; step > 0; step >>= 1) {
                const float need = sh_thr[lvl + step] * pmax;
                if (P >= need) lvl += step;
              }
            }
            col = sh_cmap[lvl];
          }
        }
        const int64_t g0 = ((int64_t)y * W + xs) * 3;
        const int p = (int)((base + (uintptr_t)g0) & 3);
        unsigned char* d = (unsigned char*)sh_pix + rr * (SH_PITCH * 4) + p + 3 * px;
        d[0] = (unsigned char)col;
        d[1] = (unsigned char)(col >> 8);
        d[2] = (unsigned char)(col >> 16);
      }
    }
    __syncthreads();
    for (int s = tid; s < SH_RC * SH_PITCH; s += SH_THREADS) {
      const int rr = s / SH_PITCH, i = s - rr * SH_PITCH;
      const int y = yc + rr;
      if (y >= ye) break;
      const int64_t g0 = ((int64_t)y * W + xs) * 3;
      const int p = (int)((base + (uintptr_t)g0) & 3);
      const int b0 = 4 * i, end = p + 3 * rw;
      const int lo = b0 > p ? b0 : p, hi = b0 + 4 < end ? b0 + 4 : end;
      if (lo >= hi) continue;
      unsigned char* dst = img + (g0 - p + b0);          // 4-byte aligned
      if (hi - lo == 4) {
        *(uint32_t*)dst = sh_pix[s];
      } else {
        const unsigned char* src = (const unsigned char*)sh_pix + rr * (SH_PITCH * 4);
        for (int k = lo; k < hi; ++k) dst[k - b0] = src[k];
      }
    }
    __syncthreads();
  }
}

extern "C" int ag_sheet_render(const float* wave, long long ld, const long long* lens, int L, const float* power,
                               const int32_t* nframes, int F, int B, const float* thresholds, const unsigned char* cmap,
                               unsigned bg, unsigned paper, unsigned ink, int cols, int Hw, int gutter, unsigned char* img, int H,
                               int W, void* stream) {
  AG_REQUIRE(wave && power && nframes && thresholds && cmap && img,
             "ag_sheet_render: null wave, power, nframes, thresholds, cmap or img");
  AG_REQUIRE(B > 0 && F > 0 && L > 0, "ag_sheet_render: B %d, F %d, L %d: all must be positive", B, F, L);
  AG_REQUIRE(L <= (1 << 30), "ag_sheet_render: clips of %d samples: at most 2^30", L);
  AG_REQUIRE(ld >= L, "ag_sheet_render: rows of %d samples at a pitch of %lld", L, ld);
  AG_REQUIRE(Hw >= 3 && Hw <= SH_MAX_STRIP, "ag_sheet_render: a wave strip of %d rows: 3 .. %d", Hw, SH_MAX_STRIP);
  AG_REQUIRE(gutter >= 0 && gutter <= SH_MAX_GUTTER, "ag_sheet_render: a gutter of %d pixels: 0 .. %d", gutter, SH_MAX_GUTTER);
  AG_REQUIRE(cols > 0 && H > 0 && W > 0, "ag_sheet_render: %d tiles across an image of %d x %d", cols, H, W);
  const long long Wt = ((long long)L + 127) / 128, Ht = (long long)Hw + SH_BINS;
  const long long rows = ((long long)H - gutter) / (Ht + gutter);
  AG_REQUIRE(gutter + (long long)cols * (Wt + gutter) == W && gutter + rows * (Ht + gutter) == H && rows * cols >= B,
             "ag_sheet_render: %d tiles of %lld x %lld, %d across with a gutter of %d, do not fit an image of %d x %d exactly "
             "(sheet.sheet_geometry)", B, Ht, Wt, cols, gutter, H, W);
  AG_REQUIRE(rows * cols <= 65535, "ag_sheet_render: %lld grid cells: at most 65535", rows * cols);
  const dim3 grid((unsigned)ag_cdiv64(Wt, SH_TC), (unsigned)(rows * cols));
  ag_note_kernel("sheet_render_kernel");
  hipLaunchKernelGGL(sheet_render_kernel, grid, dim3(SH_THREADS), 0, (hipStream_t)stream, wave, (int64_t)ld,
                     (const int64_t*)lens, L, power, nframes, F, B, thresholds, cmap, (uint32_t)bg, (uint32_t)paper, (uint32_t)ink,
                     cols, Hw, gutter, img, W);
  AG_CHECK_LAUNCH("ag_sheet_render");
  return AG_OK;
}

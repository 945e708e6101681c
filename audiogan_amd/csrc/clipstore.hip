// clipstore.hip -- ag_clip_facts, ag_clip_gather: the loader's minibatch assembled on the device from a packed store of
// every clip (audiogan_amd/dataset.py: DeviceWordStore, ClipBatch; contract in include/audiogan_hip.h).  They stand where
// the reference's pick_word scans for the last non-zero sample, peak-normalises and stacks float64 rows on the host at
// every draw (dataset.py:48-77).  fp32 whatever ag_set_precision says, no atomics, no workspace, no LDS in the gather.
//
// The store: clip c is bank[start[c] : start[c] + cap[c]]; start is int64 (the bank may exceed 2^31 floats) and a multiple
// of 4 floats, the bank 16-byte aligned and a multiple of 4 floats long, so the 16-byte load at t % 4 == 0, t < cap never
// leaves it.  What such a load brings from beyond cap (padding, or nothing the caller wrote) is masked, never used.
//
// Both kernels move bytes and do next to nothing with them: a lane's access is 16 bytes, a wave's 1 KiB of consecutive
// addresses.  ag_clip_gather reads and writes about 10 MB each at 64 x 40000; every sample costs one correctly rounded
// division, which stays far below the time of its 8 bytes.
#include "common.h"

#define CS_THREADS 256
#define CS_PER 4
#define CS_TILE (CS_THREADS * CS_PER)

typedef unsigned cs_u4 __attribute__((ext_vector_type(4)));

// ---- ag_clip_facts: one workgroup per clip ---------------------------------------------------------------------------------
// |x| as bits: for anything but a NaN the order of the bit patterns is the order of the values, every NaN lies above +inf,
// and a denormal is what it is whatever the mode a float compare would run in.  The largest pattern IS the peak: a NaN if
// there is one, else +inf if there is one, else max |x|.
__global__ __launch_bounds__(CS_THREADS) void clip_facts_kernel(const float* __restrict__ bank, const int64_t* __restrict__ start,
                                                                const int32_t* __restrict__ cap, int32_t* __restrict__ n_out,
                                                                float* __restrict__ peak_out) {
  __shared__ unsigned sh[2 * (CS_THREADS / AG_WAVE)];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t cp = cap[c];
  const cs_u4* src = (const cs_u4*)(bank + start[c]);
  unsigned last = 0, top = 0;          // last: index after the last non-zero sample (cap < 2^31)
  for (int64_t t = (int64_t)tid * CS_PER; t < cp; t += CS_TILE) {
    const cs_u4 v = src[t >> 2];
#pragma unroll
    for (int k = 0; k < CS_PER; ++k) {
      const unsigned a = v[k] & 0x7fffffffu;
      if (t + k < cp && a) {
        last = (unsigned)(t + k + 1);          // (k ascending: the thread's largest so far)
        top = a > top ? a : top;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = (unsigned)__shfl_xor((int)last, o, AG_WAVE), t2 = (unsigned)__shfl_xor((int)top, o, AG_WAVE);
    last = l2 > last ? l2 : last;
    top = t2 > top ? t2 : top;
  }
  const int lane = tid & (AG_WAVE - 1), wid = tid / AG_WAVE;
  if (lane == 0) {
    sh[2 * wid] = last;
    sh[2 * wid + 1] = top;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < CS_THREADS / AG_WAVE; ++w) {
      last = sh[2 * w] > last ? sh[2 * w] : last;
      top = sh[2 * w + 1] > top ? sh[2 * w + 1] : top;
    }
    n_out[c] = (int32_t)last;
    peak_out[c] = __uint_as_float(top);
  }
}

extern "C" int ag_clip_facts(const float* bank, const long long* start, const int32_t* cap, int32_t* n_out, float* peak_out,
                             long long n_clips, void* stream) {
  AG_REQUIRE(n_clips >= 0 && n_clips <= 0x7fffffffLL, "ag_clip_facts: %lld clips: 0 .. 2^31 - 1", n_clips);
  if (n_clips == 0) return AG_OK;
  AG_REQUIRE(bank && start && cap && n_out && peak_out, "ag_clip_facts: null bank, start, cap, n_out or peak_out");
  AG_REQUIRE(((uintptr_t)bank & 15) == 0, "ag_clip_facts: the bank must be 16-byte aligned");
  ag_note_kernel("clip_facts_kernel");
  hipLaunchKernelGGL(clip_facts_kernel, dim3((unsigned)n_clips), dim3(CS_THREADS), 0, (hipStream_t)stream, bank,
                     (const int64_t*)start, cap, n_out, peak_out);
  AG_CHECK_LAUNCH("ag_clip_facts");
  return AG_OK;
}

// ---- ag_clip_gather: grid (ceil(L_out / 1024), B) --------------------------------------------------------------------------
// VEC: out is 16-byte aligned and ld_out % 4 == 0, so column t0 = 4 (256 blockIdx.x + tid) of any row is: one 16-byte load,
// one 16-byte store; the row's last group, when L_out % 4 != 0, stores its 1 - 3 samples one by one.  Otherwise thread tid
// takes samples tid, tid + 256, .. of the tile, four 4-byte accesses whose lanes are neighbours.
template <int VEC>
__global__ __launch_bounds__(CS_THREADS) void clip_gather_kernel(const float* __restrict__ bank, const int64_t* __restrict__ start,
                                                                 const int32_t* __restrict__ n, const float* __restrict__ peak,
                                                                 const int64_t* __restrict__ ids, float* __restrict__ out,
                                                                 int64_t ld_out, int L_out, int64_t* __restrict__ len_out,
                                                                 int frame) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t c = ids[b];
  const int nc = n[c];
  const int m = nc < L_out ? nc : L_out;          // samples of the clip that reach the row
  if (blockIdx.x == 0 && tid == 0 && len_out)
    len_out[b] = frame > 0 ? ((int64_t)nc + frame - 1) / frame * frame : (int64_t)nc;
  const float* src = bank + start[c];
  float* row = out + (int64_t)b * ld_out;
  const float pk = peak[c];          // (read by every thread; used only where t < m, and m > 0 means pk > 0)
  const int64_t tile0 = (int64_t)blockIdx.x * CS_TILE;          // int64: L_out may be within 1024 of 2^31
  if (VEC) {
    const int64_t t0 = tile0 + tid * CS_PER;
    if (t0 >= L_out) return;
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    if (t0 < m) {          // t0 % 4 == 0 and t0 < n[c] <= cap[c]: inside the bank
      const f32x4 v = *(const f32x4*)(src + t0);
#pragma unroll
      for (int k = 0; k < CS_PER; ++k) y[k] = t0 + k < m ? __fdiv_rn(v[k], pk) : 0.f;
    }
    if (t0 + CS_PER <= L_out) {
      *(f32x4*)(row + t0) = y;
    } else {
#pragma unroll
      for (int k = 0; k < CS_PER; ++k)
        if (t0 + k < L_out) row[t0 + k] = y[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CS_PER; ++k) {
      const int64_t t = tile0 + k * CS_THREADS + tid;
      if (t < L_out) row[t] = t < m ? __fdiv_rn(src[t], pk) : 0.f;
    }
  }
}

extern "C" int ag_clip_gather(const float* bank, const long long* start, const int32_t* n, const float* peak,
                              const long long* ids, int B, float* out, long long ld_out, int L_out, long long* len_out,
                              int frame, void* stream) {
  AG_REQUIRE(B >= 0 && B <= 65535 && L_out >= 0 && frame >= 0, "ag_clip_gather: B %d (0 .. 65535), L_out %d, frame %d", B,
             L_out, frame);
  if (B == 0) return AG_OK;
  AG_REQUIRE(bank && start && n && peak && ids && out, "ag_clip_gather: null bank, start, n, peak, ids or out");
  AG_REQUIRE(ld_out >= L_out, "ag_clip_gather: rows of %d samples at a pitch of %lld", L_out, ld_out);
  AG_REQUIRE(((uintptr_t)bank & 15) == 0, "ag_clip_gather: the bank must be 16-byte aligned");
  const int vec = ((uintptr_t)out & 15) == 0 && (ld_out & 3) == 0;
  const dim3 grid((unsigned)(L_out > 0 ? ag_cdiv64(L_out, CS_TILE) : 1), (unsigned)B);
  if (vec) {
    ag_note_kernel("clip_gather_kernel<1>");
    hipLaunchKernelGGL(clip_gather_kernel<1>, grid, dim3(CS_THREADS), 0, (hipStream_t)stream, bank, (const int64_t*)start, n,
                       peak, (const int64_t*)ids, out, (int64_t)ld_out, L_out, (int64_t*)len_out, frame);
  } else {
    ag_note_kernel("clip_gather_kernel<0>");
    hipLaunchKernelGGL(clip_gather_kernel<0>, grid, dim3(CS_THREADS), 0, (hipStream_t)stream, bank, (const int64_t*)start, n,
                       peak, (const int64_t*)ids, out, (int64_t)ld_out, L_out, (int64_t*)len_out, frame);
  }
  AG_CHECK_LAUNCH("ag_clip_gather");
  return AG_OK;
}

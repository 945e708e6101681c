// front_stack.hip -- the stacked generator front (2 to 8 LSTMCell layers under one projection) as ONE persistent launch per
// direction: gfront_stack_fwd_kernel and gfront_stack_bwd_kernel.  The one-layer front is front_persist.hip; the blocks of the
// frame loops that both share are in front_parts.h, the hand-off protocol in persist_common.h.
#include "front_parts.h"

// ------------------------------------------------------------------------------------------
// The STACKED front (audiogan.py:382-385, :441-442: --rnng_layers LSTMCell layers under one projection) as ONE persistent
// launch: gfront_persist_fwd_kernel's design with one more coordinate.  LSTMCell only, fp32 MFMA only (AG_PREC_BF16: both
// operands of all three products rounded in registers), training and generation mode.
//
//   workgroup (l, rt, ut): layer l, 32 clips, 8 hidden units of that layer.  nl * nrt * S/8 workgroups, all co-resident.
//   layer 0   : as the one-layer kernel - the h part on its own h0_{t-1}, the x part on x_{t-1} behind the projection flags,
//               pre_t from gates[0]; the workgroups ut < NB also keep phase B (their [16 x 16] tile of x_t) and, in generation
//               mode, ut < 2 the stop head - but phase B waits for and reads the TOP layer's h_t.  (W_p stays on layer 0:
//               its x panel is the narrow one, so these workgroups have the registers.)
//   layer l>=1: two resident [4S, S] panels, W_hh_l and W_ih_l.  Frame t: the h part on its own h_{l,t-1} (may start before
//               anything of frame t exists), wait until the S/8 flags of layer l-1 reach t+1, the input part on h_{l-1,t}, LDS
//               sum, cell, h_{l,t} published.  Pre-activation: the time-invariant b_ih_l + b_hh_l, 4 values per thread.
//   Both panels of a workgroup share one register array beside W_hh (w2): layer 0 keeps W_x in its first FS/64 rows and W_p
//   behind them, an upper layer fills all S/64 rows with W_ih_l.
//
// Exchange: one h buffer per layer [2 parities][nrt][S/8][32][8] and the x buffer of the padded panel width; flags
// [nl][nrt][S/8] h flags, then [nrt][NB] x flags, all counting frames.  Hand-offs as in every persistent launch (persist_common.h).
//
// Two parities suffice.  Everything below is per row tile.  Write h_{l,t+2} (it replaces h_{l,t}) happens after the writer
// has seen (a) every flag of its own layer at t+2 and (b) l = 0: every x flag at t+2, l >= 1: every flag of layer l-1 at t+3.
// (b) implies x_{t+1} complete: for l >= 1 by descending to layer 0, whose frame t+2 needs it.  x_{t+1} complete means every
// top-layer workgroup has published h_{top,t+1}, which needed every workgroup of layer top-1 to have published h_{.,t+1}, and
// so on down: every workgroup of EVERY layer is past its frame t, and the projection tiles are past phase B of frame t+1.
// The readers of h_{l,t} are layer l in the h part of frame t+1 (done: (a)), layer l+1 in the input part of frame t and the
// projection in phase B of frame t (done: above).  Likewise x_{t+2} is written after every top flag reached t+3, hence after
// every layer-0 workgroup published h_{0,t+2}, i.e. finished reading x_t in frame t+1.
//
// Generation mode: the exit test of the one-layer kernel, taken at the top of a frame by every workgroup of every layer from
// the same write-once words; the decisions of frame t-1-GEN_LAG are final before any layer can have finished frame t-1, so
// the test never waits on an upper layer either.  Every workgroup therefore runs the same frames and nobody waits for a
// flag that is never published.
// ------------------------------------------------------------------------------------------
struct FrontStackP {
  float* gates[FRONT_MAX_LAYERS];        // [T,B,4S] per layer.  [0]: in pre, training: out activated; [l>=1]: training out
  float* hs[FRONT_MAX_LAYERS];           // training: [T,B,S]
  float* cs[FRONT_MAX_LAYERS];           // training: [T+1,B,S]  (cs[l][0] is written 0 by the launch)
  const float* whh[FRONT_MAX_LAYERS];    // [4S,S]
  const float* win[FRONT_MAX_LAYERS];    // [0]: W_ih_0[:, :fs] with pitch ldwx; [l>=1]: W_ih_l [4S,S]
  const float* bias[FRONT_MAX_LAYERS];   // [l>=1]: b_ih_l + b_hh_l [4S]
  const float* wp;     // [fs, S]
  const float* bp;     // [fs]
  float* x;            // [B, T*fs], row pitch ldx
  float* xt;           // training, optional [T,B,fs]
  int64_t ldx;
  float* hx;           // exchange: h   [nl][2][nrt][S/8][32][8]
  float* xx;           // exchange: x   [2][nrt][FS/8][32][8]
  PersistCtl ctl;
  int T, B, ldwx, nrt, rb, fs, nl;
  // generation mode (as FrontGenP)
  const float* ws;
  const float* bs;
  const float* u;
  float* s;
  int64_t lds;
  int* first;
  int* t_run;
};

template <int S, int FS, int GEN>
__global__ __launch_bounds__(512) void gfront_stack_fwd_kernel(const FrontStackP p) {
  constexpr int NUT = S / 8;
  constexpr int QH = S / 64, QX = FS / 64;
  constexpr int NBMAX = 2 * (FS / 16);
  constexpr int UP = S / 128;
  // 8-k groups of an [S]-deep product loaded per batch: with two [4S, S] panels resident (128 VGPRs at S = 1024) a whole
  // wave's share of an h row (another 64) does not fit beside them
  // (generation mode: the stop head's state on top - batches of 4)
  constexpr int CH = QH > 8 ? (GEN == 1 ? 4 : 8) : QH;
  static_assert(S % 128 == 0 && FS % 64 == 0 && NBMAX <= NUT && NBMAX <= 64 && QX + UP <= QH && QH % CH == 0, "unsupported front shape");
  __shared__ float red[8 * 1024];
  __shared__ int s_dead;
  __shared__ int s_exit;
  const int T = p.T, B = p.B, fs = p.fs, nl = p.nl;
  const int NB = 2 * ((fs + 15) >> 4);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5, li = lane & 15, g = lane >> 4;
  if (tid == 0) { s_dead = 0; s_exit = 0; }
  __syncthreads();
  const int rt = blockIdx.x % p.nrt, rest = blockIdx.x / p.nrt;
  const int l = rest / NUT, ut = rest - l * NUT;
  const bool l0 = l == 0;
  const int l2 = l0 ? nl - 1 : l - 1;        // the other layer this workgroup reads: the top one (projection) / the one below
  const int u0 = ut * 8, row0 = rt * 32;

  // ---- resident panels (B operands).  Gate column j = gate (j>>3), unit u0 + (j&7).
  const bool bwg = l0 && ut < NB;            // this workgroup also owns a projection tile
  const int bsub = ut & 1, bcol0 = (ut >> 1) * 16;
  const bool wpv = bwg && bcol0 + li < fs;   // this lane's row of W_p exists (rows past fs read as zeros)
  float wh[QH][4], w2[QH][4];
  {
    const int wrow = (l31 >> 3) * S + u0 + (l31 & 7);
    const float* whh = p.whh[l];
    const float* win = p.win[l];
#pragma unroll
    for (int q = 0; q < QH; ++q) {
      const f32x4 v = ag_rbf4_if(*reinterpret_cast<const f32x4*>(whh + (int64_t)wrow * S + (wid * QH + q) * 8 + 4 * hh), p.rb);
#pragma unroll
      for (int e = 0; e < 4; ++e) wh[q][e] = v[e];
    }
    if (l0) {
#pragma unroll
      for (int q = 0; q < QX; ++q) {
        const int kx = (wid * QX + q) * 8 + 4 * hh;       // (k >= fs: zeros - what lies there in the row are the z/c weights)
        const f32x4 v = kx >= fs ? f32x4{0.f, 0.f, 0.f, 0.f}
                                 : ag_rbf4_if(*reinterpret_cast<const f32x4*>(win + (int64_t)wrow * p.ldwx + kx), p.rb);
#pragma unroll
        for (int e = 0; e < 4; ++e) w2[q][e] = v[e];
      }
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        const f32x4 v = wpv ? ag_rbf4_if(*reinterpret_cast<const f32x4*>(p.wp + (int64_t)(bcol0 + li) * S + (wid * UP + u) * 16 + 4 * g), p.rb)
                            : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) w2[QX + u][e] = v[e];
      }
#pragma unroll
      for (int q = QX + UP; q < QH; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) w2[q][e] = 0.f;
    } else {
#pragma unroll
      for (int q = 0; q < QH; ++q) {
        const f32x4 v = ag_rbf4_if(*reinterpret_cast<const f32x4*>(win + (int64_t)wrow * S + (wid * QH + q) * 8 + 4 * hh), p.rb);
#pragma unroll
        for (int e = 0; e < 4; ++e) w2[q][e] = v[e];
      }
    }
  }
  // generation mode: the stop head's weight in LDS, on the stop workgroups only
  const bool swg = GEN == 1 && l0 && ut < 2;
  __shared__ __attribute__((aligned(16))) float wsl[GEN == 1 ? S : 4];
  float bsv = 0.f;
  if constexpr (GEN == 1) {
    if (swg) {
      for (int k = tid; k < S; k += 512) wsl[k] = p.ws[k];
      bsv = p.bs[0];
    }
    __syncthreads();
  }

  unsigned* flag_h = p.ctl.hdr + PS_FLAG_OFF + (l * p.nrt + rt) * NUT;       // this layer's h flags
  unsigned* flag_2 = p.ctl.hdr + PS_FLAG_OFF + (l2 * p.nrt + rt) * NUT;      // the other layer's
  unsigned* flag_x = p.ctl.hdr + PS_FLAG_OFF + nl * p.nrt * NUT + rt * NB;
  const int64_t hgs = (int64_t)NUT * 32 * 8, xgs = (int64_t)(FS / 8) * 32 * 8;     // floats per (parity, rt)
  const int hbytes = (int)(2 * p.nrt * hgs * 4);                                   // one layer's h buffer
  __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc(p.hx + (int64_t)l * 2 * p.nrt * hgs, 0, hbytes, 0x00020000);
  __amdgpu_buffer_rsrc_t h2r = __builtin_amdgcn_make_buffer_rsrc(p.hx + (int64_t)l2 * 2 * p.nrt * hgs, 0, hbytes, 0x00020000);
  __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(p.xx, 0, (int)(2 * p.nrt * xgs * 4), 0x00020000);

  // phase A epilogue role: thread (clip row, unit), tid < 256
  const int erow = tid >> 3, euu = tid & 7;
  const int em = row0 + erow, eu = u0 + euu;
  const bool epi = tid < 256 && em < B;
  const int ee = (erow & 3) + 4 * (erow >> 3), ehq = (erow >> 2) & 1;
  float creg = 0.f;
  // phase B epilogue role: thread (clip row within the 16-row subtile, column), tid < 256
  const int brow = tid >> 4, bcl = tid & 15;
  const int bm = row0 + 16 * bsub + brow;
  const bool bcv = bcol0 + bcl < fs;
  const float bbias = (bwg && tid < 256 && bcv) ? p.bp[bcol0 + bcl] : 0.f;
  bool alive = true;
  // fs < FS: the ownerless 8-column groups of the x exchange buffer are zeroed once by the projection workgroups (as in
  // gfront_persist_fwd_kernel: drained before the barrier in front of the workgroup's first x flag)
  if (bwg && tid < 256) {
    for (int gp = NB + ut; gp < FS / 8; gp += NB) {
#pragma unroll
      for (int par = 0; par < 2; ++par)
        __builtin_amdgcn_raw_buffer_store_b32(0u, xr, (unsigned)(((int64_t)(par * p.nrt + rt) * xgs + (int64_t)gp * 256 + tid) * 4), 0, 16);
    }
  }

  // the epilogue's pre-activations: layer 0 per frame from gates[0] (requested at the end of the previous frame), an upper
  // layer once
  float* const gl = p.gates[l];
  float* const hsl = GEN == 0 ? p.hs[l] : nullptr;
  float* const csl = GEN == 0 ? p.cs[l] : nullptr;
  float pre4[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_pre = [&](int tt) {
    if (epi && l0) {
      const float* pr = gl + ((int64_t)tt * B + em) * 4 * S + eu;
      pre4[0] = pr[0]; pre4[1] = pr[S]; pre4[2] = pr[2 * S]; pre4[3] = pr[3 * S];
    }
  };
  if (l0) load_pre(0);
  else if (epi) {
    const float* bl = p.bias[l] + eu;
    pre4[0] = bl[0]; pre4[1] = bl[S]; pre4[2] = bl[2 * S]; pre4[3] = bl[3 * S];
  }
  // generation mode: thread tid < 16 of a stop workgroup owns clip sm of its subtile (first stop, next uniform)
  const int nsub = 2 * p.nrt, sub = 2 * rt + (ut & 1);
  unsigned* gen_done = p.ctl.hdr + PS_GEN_OFF;
  unsigned* gen_all = gen_done + 8;
  const int sm = row0 + 16 * (ut & 1) + tid;
  const bool sthr = swg && tid < 16 && sm < B;
  int fst = T, t_ran = T;
  bool all_pub = false;
  float ureg = 1.f;
  // (the uniforms through a buffer descriptor: a per-thread 64-bit pointer kept over the whole loop was the one value the
  // S = 1024 form spilled)
  __amdgpu_buffer_rsrc_t ur = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.u), 0, GEN == 1 ? T * B * 4 : 0, 0x00020000);
  if constexpr (GEN == 1) {
    if (sthr) ureg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ur, (unsigned)(sm * 4), 0, 0));
  }
  for (int t = 0; t < T; ++t) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (t > 0) {
      const int par = (t - 1) & 1;
      bool ex = false;
      if constexpr (GEN == 1) {
        // exit test on the final decisions of frame t - 1 - GEN_LAG (folded into the barrier of the h wait below)
        if (wid == 0) {
          if (t > GEN_LAG && alive) {
            const unsigned want = (unsigned)(t - GEN_LAG);
            alive = ps_wait_flags(p.ctl, gen_done, nsub, want, lane);
            if (!alive) s_dead = 1;
            else {
              const unsigned a = lane < nsub ? __hip_atomic_load(gen_all + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1u;
              ex = __all(a != 0u && a <= want);
            }
          }
          if (lane == 0) s_exit = ex ? 1 : 0;
        }
      }
      // ---- h part: this layer's h_{t-1}
      if (wid == 0 && alive && !ex) {
        alive = ps_wait_flags(p.ctl, flag_h, NUT, (unsigned)t, lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      if constexpr (GEN == 1) {
        if (s_exit) { t_ran = t; break; }
      }
      {
        const unsigned ab = (unsigned)(((int64_t)(par * p.nrt + rt) * hgs + (int64_t)l31 * 8 + 4 * hh) * 4);
#pragma unroll
        for (int qb = 0; qb < QH; qb += CH) {
          u32x4 a[CH];
#pragma unroll
          for (int q = 0; q < CH; ++q) a[q] = __builtin_amdgcn_raw_buffer_load_b128(hr, ab + (unsigned)((wid * QH + qb + q) * 32 * 32), 0, 16);
          if (p.rb) {
#pragma unroll
            for (int q = 0; q < CH; ++q)
#pragma unroll
              for (int e = 0; e < 4; ++e) a[q][e] = __float_as_uint(ag_rbf(__uint_as_float(a[q][e])));
          }
#pragma unroll
          for (int q = 0; q < CH; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[q][e]), wh[qb + q][e], acc, 0, 0, 0);
        }
      }
      // ---- layer 0: the x part on x_{t-1}
      if (l0) {
        if (wid == 0 && alive) {
          alive = ps_wait_flags<true>(p.ctl, flag_x, NB, (unsigned)t, lane);
          if (!alive) s_dead = 1;
        }
        __syncthreads();
        const unsigned ab = (unsigned)(((int64_t)(par * p.nrt + rt) * xgs + (int64_t)l31 * 8 + 4 * hh) * 4);
        u32x4 a[QX];
#pragma unroll
        for (int q = 0; q < QX; ++q) a[q] = __builtin_amdgcn_raw_buffer_load_b128(xr, ab + (unsigned)((wid * QX + q) * 32 * 32), 0, 16);
        if (p.rb) {
#pragma unroll
          for (int q = 0; q < QX; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[q][e] = __float_as_uint(ag_rbf(__uint_as_float(a[q][e])));
        }
#pragma unroll
        for (int q = 0; q < QX; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[q][e]), w2[q][e], acc, 0, 0, 0);
      }
    }
    // ---- layer l >= 1: the input part on h_{l-1,t}
    if (!l0) {
      if (wid == 0 && alive) {
        alive = ps_wait_flags(p.ctl, flag_2, NUT, (unsigned)(t + 1), lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      const unsigned ab = (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + (int64_t)l31 * 8 + 4 * hh) * 4);
#pragma unroll
      for (int qb = 0; qb < QH; qb += CH) {
        u32x4 a[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) a[q] = __builtin_amdgcn_raw_buffer_load_b128(h2r, ab + (unsigned)((wid * QH + qb + q) * 32 * 32), 0, 16);
        if (p.rb) {
#pragma unroll
          for (int q = 0; q < CH; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[q][e] = __float_as_uint(ag_rbf(__uint_as_float(a[q][e])));
        }
#pragma unroll
        for (int q = 0; q < CH; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[q][e]), w2[qb + q][e], acc, 0, 0, 0);
      }
    }
    front_acc_to_red(red, wid, lane, acc);
    __syncthreads();
    float hreg = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f;
    if (epi) {
      float g4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float s = pre4[q];
        if (t > 0 || !l0) {
#pragma unroll
          for (int w = 0; w < 8; ++w) s += red[w * 1024 + ee * 64 + 32 * ehq + 8 * q + euu];
        }
        g4[q] = s;
      }
      ig = ag_sigmoid(g4[0]); fg = ag_sigmoid(g4[1]); gg = tanhf(g4[2]); og = ag_sigmoid(g4[3]);
      creg = fg * creg + ig * gg;
      hreg = og * tanhf(creg);
      if (s_dead) creg = hreg = ig = __builtin_nanf("");             // a wait timed out: poison instead of garbage
    }
    if (tid < 256) {
      // publish h_{l,t} (rows past the batch: zeros, so that the exchange buffer stays defined)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hreg), hr,
          (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + ((int64_t)ut * 32 + erow) * 8 + euu) * 4), 0, 16);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
      __hip_atomic_store(flag_h + ut, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 1 < T) load_pre(t + 1);
    if (GEN == 0 && epi) {      // (the generation mode keeps no history)
      float* pr = gl + ((int64_t)t * B + em) * 4 * S + eu;
      pr[0] = ig; pr[S] = fg; pr[2 * S] = gg; pr[3 * S] = og;
      if (t == 0) csl[(int64_t)em * S + eu] = 0.f;               // c_0 = 0: written here, so the caller need not fill it
      csl[((int64_t)(t + 1) * B + em) * S + eu] = creg;
      hsl[((int64_t)t * B + em) * S + eu] = hreg;
    }
    // ---- phase B (layer 0, ut < NB): this workgroup's tile of x_t = tanh(h_top,t W_p^T + b)
    if (bwg) {
      if (wid == 0 && alive) {
        alive = ps_wait_flags(p.ctl, flag_2, NUT, (unsigned)(t + 1), lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      f32x4 pacc = {0.f, 0.f, 0.f, 0.f};
      float sdot = 0.f;          // (generation mode, stop workgroups) this lane's part of h_t . w_s
      {
        // A = h_top,t rows of the 16-clip subtile: lane (clip li, k slot g) takes k = 16u + 4g .. +3 = unit tile 2u + (g>>1), half g&1
        const unsigned ab = (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + (int64_t)(16 * bsub + li) * 8 + 4 * (g & 1)) * 4);
        u32x4 a[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u)
          a[u] = __builtin_amdgcn_raw_buffer_load_b128(h2r, ab + (unsigned)((2 * (wid * UP + u) + (g >> 1)) * 32 * 32), 0, 16);
        if constexpr (GEN == 1) {
          if (swg) {     // (the stop logit from the unrounded h_t)
#pragma unroll
            for (int u = 0; u < UP; ++u) {
              const f32x4 w = *reinterpret_cast<const f32x4*>(wsl + 16 * (wid * UP + u) + 4 * g);
#pragma unroll
              for (int e = 0; e < 4; ++e) sdot = fmaf(__uint_as_float(a[u][e]), w[e], sdot);
            }
          }
        }
        if (p.rb) {
#pragma unroll
          for (int u = 0; u < UP; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[u][e] = __float_as_uint(ag_rbf(__uint_as_float(a[u][e])));
        }
#pragma unroll
        for (int u = 0; u < UP; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[u][e]), w2[QX + u][e], pacc, 0, 0, 0);
      }
      // 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + e   (red is free again: the gate sums were consumed above)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wid * 256 + (4 * g + e) * 16 + li] = pacc[e];
      if constexpr (GEN == 1) {
        if (swg) {
          sdot += __shfl_xor(sdot, 16);
          sdot += __shfl_xor(sdot, 32);
          if (g == 0) red[2048 + wid * 16 + li] = sdot;
        }
      }
      __syncthreads();
      if (tid < 256) {
        float v = bbias;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += red[w * 256 + tid];
        v = s_dead ? __builtin_nanf("") : tanhf(v);
        const int col = bcol0 + bcl;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(bm < B && bcv ? v : 0.f), xr,
            (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * xgs + ((int64_t)(col >> 3) * 32 + 16 * bsub + brow) * 8 + (col & 7)) * 4), 0, 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (bm < B && bcv) {
          p.x[(int64_t)bm * p.ldx + (int64_t)t * fs + col] = v;
          if (GEN == 0 && p.xt) p.xt[((int64_t)t * B + bm) * fs + col] = v;
        }
        if constexpr (GEN == 1) {
          if (swg && wid == 0) {
            // stop logit and draw of clip sm; then the subtile's words, published before the x flag below
            if (sthr) {
              float sv = bsv;
#pragma unroll
              for (int w = 0; w < 8; ++w) sv += red[2048 + w * 16 + tid];
              if (s_dead) sv = __builtin_nanf("");
              p.s[(int64_t)sm * p.lds + t] = sv;
              if (fst == T && ureg < ag_sigmoid(sv)) fst = t + 1;
            }
            const bool all = __all(!sthr || fst <= t + 1);      // (clips past the batch count as stopped)
            if (tid == 0) {
              if (all && !all_pub) {
                __hip_atomic_store(gen_all + sub, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                all_pub = true;
              }
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // gen_all lands before gen_done says "frame t is final"
              __hip_atomic_store(gen_done + sub, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (sthr && t + 1 < T) ureg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ur, (unsigned)(((t + 1) * B + sm) * 4), 0, 0));
          }
        }
      }
      __syncthreads();
      if (tid == 0) __hip_atomic_store(flag_x + ut, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if constexpr (GEN == 1) {
    if (sthr) p.first[sm] = fst;
    if (blockIdx.x == 0 && tid == 0) *p.t_run = t_ran;
  }
}

static bool front_stack_shape_ok(int B, int S, int fs, int nl, int n_cu) {
  if (nl < 2 || nl > FRONT_MAX_LAYERS) return false;
  if (!front_fs_ok(S, fs)) return false;
  if (B < 1 || B > 64) return false;
  if (n_cu > 256) n_cu = 256;
  return nl * ag_cdiv(B, 32) * (S / 8) <= n_cu;
}

extern "C" int ag_gfront_stack_ok(int B, int S, int fs, int nl, int n_cu) { return front_stack_shape_ok(B, S, fs, nl, n_cu) ? 1 : 0; }

extern "C" int64_t ag_gfront_stack_ws_bytes(int B, int S, int fs, int nl) {
  // (one h buffer per layer; the x buffer has the padded panel width whatever fs is)
  const int w = front_fs_ok(S, fs) ? front_panel(S) : fs;
  return PS_STICKY_BYTES + PS_HDR_BYTES + (int64_t)2 * ag_cdiv(B, 32) * 32 * ((int64_t)(nl > 0 ? nl : 0) * S + w) * 4;
}

template <int S, int FS, int GEN>
static void front_stack_launch(const FrontStackP& p, int grid, hipStream_t st) {
  static const AgKernelName name("gfront_stack_fwd_kernel", {S, FS, GEN});
  ag_note_kernel(name.s);
  hipLaunchKernelGGL((gfront_stack_fwd_kernel<S, FS, GEN>), dim3(grid), dim3(512), 0, st, p);
}

// The frame loop of a front with 2 to 8 LSTMCell layers in ONE launch, training forward and generation mode.  Tensor
// contracts: ag_front_stack_args (include/audiogan_hip.h).  Shapes: ag_gfront_stack_ok.
extern "C" int ag_gfront_stack_fwd(const ag_front_stack_args* a, void* stream) {
  static const char* const who = "ag_gfront_stack_fwd";
  if (int rc = front_struct_ok(who, a, "ag_front_stack_args")) return rc;
  AG_REQUIRE(a->gen == 0 || a->gen == 1, "%s: gen must be 0 (training) or 1 (generation)", who);
  AG_REQUIRE(a->nl >= 1 && a->nl <= FRONT_MAX_LAYERS, "%s: nl = %d, the per-layer tables hold 1 to %d layers", who, a->nl, FRONT_MAX_LAYERS);
  const bool gen = a->gen == 1;
  const int nl = a->nl;
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    const FrontField f[] = {{"gates", a->gates[l], !gen || l == 0}, {"hs", a->hs[l], !gen}, {"cs", a->cs[l], !gen},
                            {"w_hh", a->w_hh[l], true}, {"w_in", a->w_in[l], true}, {"bias", a->bias[l], l > 0}};
    if (int rc = front_layer_fields_ok(who, l, nl, f)) return rc;
  }
  const FrontField fields[] = {
      {"w_p", a->w_p, true}, {"b_p", a->b_p, true}, {"x", a->x, true}, {"xt", a->xt, !gen && a->xt},      // (optional in training)
      {"w_s", a->w_s, gen}, {"b_s", a->b_s, gen}, {"u", a->u, gen}, {"s", a->s, gen}, {"first", a->first, gen},
      {"t_run", a->t_run, gen}, {"ws", a->ws, true}};
  if (int rc = front_fields_ok(who, fields)) return rc;
  const int T = a->T, B = a->B, S = a->S, fs = a->fs;
  AG_REQUIRE(T > 0, "%s: T must be positive", who);
  AG_REQUIRE(a->ldx >= (int64_t)T * fs, "%s: x row pitch smaller than a row", who);
  AG_REQUIRE(!gen || a->lds >= T, "%s: s row pitch smaller than a row", who);
  AG_REQUIRE((int64_t)T * 64 * 4 < ((int64_t)1 << 31), "%s: too many frames", who);      // (u is addressed with 32-bit byte offsets)
  if (!front_stack_shape_ok(B, S, fs, nl, a->n_cu)) {
    ag_set_error("%s: shape B=%d S=%d fs=%d nl=%d is not supported on %d CUs", who, B, S, fs, nl, a->n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  uintptr_t al = (uintptr_t)a->w_p;
  for (int l = 0; l < nl; ++l) al |= (uintptr_t)a->w_hh[l] | (uintptr_t)a->w_in[l];
  AG_REQUIRE(a->ldwx >= fs && a->ldwx % 4 == 0 && (al & 15) == 0, "%s: weights must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  FrontStackP p;
  if (int rc = persist_begin(who, a->ws, a->ws_bytes, ag_gfront_stack_ws_bytes(B, S, fs, nl), st, &p.ctl)) return rc;
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    p.gates[l] = a->gates[l]; p.hs[l] = a->hs[l]; p.cs[l] = a->cs[l];
    p.whh[l] = a->w_hh[l]; p.win[l] = a->w_in[l]; p.bias[l] = a->bias[l];
  }
  p.wp = a->w_p; p.bp = a->b_p; p.x = a->x; p.ldx = a->ldx; p.xt = a->xt;
  p.ws = a->w_s; p.bs = a->b_s; p.u = a->u; p.s = a->s; p.lds = a->lds; p.first = a->first; p.t_run = a->t_run;
  p.nrt = ag_cdiv(B, 32);
  p.hx = (float*)((char*)a->ws + PS_STICKY_BYTES + PS_HDR_BYTES);
  p.xx = p.hx + (int64_t)nl * 2 * p.nrt * 32 * S;
  p.T = T; p.B = B; p.ldwx = a->ldwx; p.fs = fs; p.nl = nl; p.rb = ag_precision() == AG_PREC_BF16;
  const int grid = nl * p.nrt * (S / 8);
  if (S == 1024) {
    if (gen) front_stack_launch<1024, 256, 1>(p, grid, st);
    else front_stack_launch<1024, 256, 0>(p, grid, st);
  } else {
    if (gen) front_stack_launch<128, 64, 1>(p, grid, st);
    else front_stack_launch<128, 64, 0>(p, grid, st);
  }
  AG_CHECK_LAUNCH(who);
  return AG_OK;
}
// ------------------------------------------------------------------------------------------
// Backward through time of a STACKED front (2 to 8 LSTMCell layers, L = nl - 1 the top one) as ONE persistent launch: the
// one-layer launch (front_persist.hip) with a layer coordinate.  Per frame t = T-1 .. 0 (every term of frame T is zero):
//   gx_t     = (dx_ext[t] + dg_{0,t+1} W_x) * (1 - x_t^2)                        -> dxt[t]
//   dh_{L,t} = dh_ext[t] + dg_{L,t+1} W_hh_L + gx_t W_p
//   dh_{l,t} = dg_{l,t+1} W_hh_l + dg_{l+1,t} W_ih_{l+1}                          l < L
//   dg_{l,t} = cell backward(dh_{l,t}, dc_{l,t+1})                                -> dgs[l][t]; dc stays in a register
// Workgroups per clip tile of 32: nl * S/16 h tiles (layer l, 16 columns of h_l) and ceil(fs/16) x tiles, the roles of the
// one-layer kernel.  An h tile keeps its [4S x 16] panel of W_hh_l in registers; the top layer's also W_p's [fs x 16]
// panel; an h tile of a layer l < L a second [4S x 16] panel, W_ih_{l+1}[:, cols].  At S = 1024 a panel is 256 KiB (128
// registers per lane): beside the first one, 15 of a wave's 32 k units of the second (60 registers) stay in registers and
// 17 lie in LDS (136 KiB beside the 16 KiB of `red`, of 160 KiB), laid out [wave][k unit][g][li][e]: lane (g, li) writes and reads
// ITS four e values as one b128 at lane * 16 bytes of a 1 KiB unit - conflict free, and private to the lane that wrote it.
// At S = 128 both panels are 16 registers.
// Chain of a frame: the x tiles publish gx_t; the top h tiles publish dg_{L,t}; each lower layer waits for every dg_{l+1,t}
// of its clip tile and publishes dg_{l,t}; then every tile forms its recurrent term of frame t-1 from its own layer's
// dg_{l,t} (the x tiles from dg_{0,t}).  nl + 1 hand-offs per frame.  Every frame has its own slot in dgs[l] / dxt, written
// once and never again, so no reader can meet a later frame's value: no parity, no second buffer; flags count frames.
// ------------------------------------------------------------------------------------------
struct FrontStackBwdP {
  const float* ga[FRONT_MAX_LAYERS];     // [T,B,4S] activated gates per layer
  const float* cs[FRONT_MAX_LAYERS];     // [T+1,B,S]
  const float* whh[FRONT_MAX_LAYERS];    // [4S,S]
  const float* win[FRONT_MAX_LAYERS];    // [0]: W_ih_0[:, :fs] with pitch ldwx; [l>=1]: W_ih_l [4S,S]
  float* dgs[FRONT_MAX_LAYERS];          // [T,B,4S] out (and exchange)
  const float* wp;     // [fs,S]
  const float* x;      // [B,T*fs], row pitch ldx
  const float* dh_ext; // [T,B,S] or NULL: lands on the top layer only
  const float* dx_ext; // [B,T*fs], row pitch lddx, or NULL
  float* dxt;          // [T,B,fs] out (and exchange)
  int64_t ldx, lddx;
  PersistCtl ctl;
  int T, B, ldwx, fs, nl;
};

// 16-k units per wave of a lower layer's second panel that lie in LDS (1 KiB each; 17 * 8 waves + `red` = 152 of 160 KiB)
#define FRONT_STACK_BWD_LDS_UNITS(NU) ((NU) > 16 ? 17 : 0)

// One body per role (ROLE 0: x tile, 1: h tile of the top layer, 2: h tile of a lower layer), so that the registers of a
// role hold only what that role keeps: the kernel branches to one of them once.
template <int S, int FS, bool RB, int ROLE>
__device__ __forceinline__ void front_stack_bwd_body(const FrontStackBwdP& p, float* red, float* w2l, int* s_dead, int bt, int ct, int l) {
  constexpr bool isx = ROLE == 0, top = ROLE == 1, low = ROLE == 2;
  constexpr int K4 = 4 * S, NU = K4 / 128;                  // 16-k units of a big product per wave
  constexpr int NHT = S / 16;
  constexpr int NP = FS >= 128 ? FS / 128 : 1;              // 16-k units of the projection product per wave
  constexpr int NL2 = FRONT_STACK_BWD_LDS_UNITS(NU);        // units of the second panel kept in LDS, per wave
  constexpr int NR2 = NU - NL2;                             // ... and in registers
  constexpr int NW2 = low ? NR2 : NP;
  const int T = p.T, B = p.B, fs = p.fs, nl = p.nl;
  const int NXT = (fs + 15) >> 4, NT = nl * NHT + NXT;      // x tiles / all tiles per clip tile
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = bt * 32;
  const int n0 = (isx ? ct - nl * NHT : ct - l * NHT) * 16; // first column inside W_hh_l / W_x
  const int64_t BG = (int64_t)B * K4, BH = (int64_t)B * S, BX = (int64_t)B * fs;

  // The panels are fetched once, with buffer loads: element [16 * unit + 4g + e][n0 + li] of a matrix of row pitch ldw is
  // at scalar offset (unit * 16 * ldw) + lane offset ((4g + e) * ldw + n0 + li) - four lane offsets serve a whole panel
  const int widu = __builtin_amdgcn_readfirstlane(wid);
  auto panel = [&](__amdgpu_buffer_rsrc_t r, int ldw, int unit, int e) {
    return ag_rbf_if(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (unsigned)(((4 * g + e) * ldw + n0 + li) * 4),
                                                                           (unsigned)(unit * 16 * ldw * 4), 0)), RB);
  };
  // resident panel: wreg[u][e] = W[(wid*NU + u)*16 + 4g + e][n0 + li]
  float wreg[NU][4];
  {
    const float* W = isx ? p.win[0] : p.whh[l];
    const int ldw = isx ? p.ldwx : S;
    const bool wv = !isx || n0 + li < fs;                   // (x tiles: columns at or past fs are the z/c weights - zeros instead)
    __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, (int)(((int64_t)(K4 - 1) * ldw + (isx ? fs : S)) * 4), 0x00020000);
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) wreg[u][e] = wv ? panel(wr, ldw, widu * NU + u, e) : 0.f;
  }
  // second panel.  Top layer: w2[u][e] = W_p[(wid*NP + u)*16 + 4g + e][n0 + li], u < NP (rows at or past fs: zeros).
  // Lower layers: W_ih_{l+1}[(wid*NU + u)*16 + 4g + e][n0 + li]: units below NR2 in w2, the others in LDS.
  const bool pw_on = top && (wid * NP * 16 < fs);
  float w2[NW2][4];
  bool pkv[NP];
  (void)w2;
#pragma unroll
  for (int u = 0; u < NP; ++u) pkv[u] = pw_on && (wid * NP + u) * 16 + 4 * g < fs;
  if constexpr (low) {
    __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.win[l + 1]), 0, K4 * S * 4, 0x00020000);
#pragma unroll
    for (int u = 0; u < NR2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) w2[u][e] = panel(wr, S, widu * NU + u, e);
    if constexpr (NL2 > 0) {
#pragma unroll
      for (int u = 0; u < NL2; ++u) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = panel(wr, S, widu * NU + NR2 + u, e);
        *reinterpret_cast<f32x4*>(&w2l[(wid * NL2 + u) * 256 + lane * 4]) = v;
      }
    }
  } else if constexpr (top) {
    __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wp), 0, fs * S * 4, 0x00020000);
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) w2[u][e] = pkv[u] ? panel(wr, S, widu * NP + u, e) : 0.f;
  }
  __syncthreads();

  unsigned* flags_t = p.ctl.hdr + PS_FLAG_OFF + bt * NT;    // [layer][h tile], then the x tiles
  unsigned* flags_own = flags_t + l * NHT;                  // the dgates this workgroup's recurrent term reads
  unsigned* flags_up = flags_t + (l + 1) * NHT;             // lower layers: the layer above
  unsigned* flags_x = flags_t + nl * NHT;
  unsigned* my_flag = flags_t + ct;
  const float* ga = p.ga[l];
  const float* c_all = p.cs[l];
  float* dg_own = p.dgs[l];
  float* dg_up = p.dgs[low ? l + 1 : l];
  // epilogue role: thread <-> (clip row, column of the tile)
  const int erow = tid >> 4, ecol = tid & 15;
  const int em = m0 + erow;
  const bool epi = em < B && (!isx || n0 + ecol < fs);      // (x tiles: columns at or past fs do not exist)
  const unsigned og4 = (unsigned)(((int64_t)em * K4 + n0 + ecol) * 4);      // this thread's byte offsets inside a frame of
  const unsigned oc4 = (unsigned)(((int64_t)em * S + n0 + ecol) * 4);       // gates / dgates, and of c / dh_ext
  // A operand rows of this lane for the two 16-clip halves (clamped: rows past the batch feed only their own, unwritten outputs)
  const int ar0 = min(m0 + li, B - 1), ar1 = min(m0 + 16 + li, B - 1);
  const unsigned o0 = (unsigned)(((int64_t)ar0 * K4 + wid * NU * 16 + 4 * g) * 4);
  const unsigned o1 = (unsigned)(((int64_t)ar1 * K4 + wid * NU * 16 + 4 * g) * 4);
  constexpr int UB = NU < 4 ? NU : 4;                       // units loaded per batch (a unit's offset rides in the scalar offset:
                                                            // added to the lane offset it would cost a register per load)
  float carry = 0.f, dcn = 0.f;
  bool alive = true;

  for (int t = T - 1; t >= 0; --t) {
    const unsigned seq = (unsigned)(T - t);
    if constexpr (isx) {
      if (epi) {
        const float dx = (p.dx_ext ? p.dx_ext[(int64_t)em * p.lddx + (int64_t)t * fs + n0 + ecol] : 0.f) + carry;
        const float xv = p.x[(int64_t)em * p.ldx + (int64_t)t * fs + n0 + ecol];
        float gx = dx * (1.f - xv * xv);
        if (*s_dead) gx = __builtin_nanf("");
        __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(p.dxt + (int64_t)t * BX, 0, (int)(BX * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(gx), orr, (unsigned)(((int64_t)em * fs + n0 + ecol) * 4), 0, 16);
      }
    } else {
      float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cp = 0.f, cn = 0.f, ext = 0.f;
      if (epi) {
        // (what the forward saved: plain cached loads, nobody writes these during the launch)
        __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ga) + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
        __amdgpu_buffer_rsrc_t cr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(c_all) + (int64_t)t * BH, 0, (int)(2 * BH * 4), 0x00020000);
        ig = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gr, og4, 0, 0));
        fg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gr, og4 + (unsigned)(S * 4), 0, 0));
        gg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gr, og4 + (unsigned)(2 * S * 4), 0, 0));
        og = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gr, og4 + (unsigned)(3 * S * 4), 0, 0));
        cp = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(cr, oc4, 0, 0));                        // c_{t-1}
        cn = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(cr, oc4, (unsigned)(BH * 4), 0));       // c_t
        if (top && p.dh_ext) {
          __amdgpu_buffer_rsrc_t er = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dh_ext) + (int64_t)t * BH, 0, (int)(BH * 4), 0x00020000);
          ext = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(er, oc4, 0, 0));
        }
      }
      if (wid == 0 && alive) {
        alive = top ? ps_wait_flags<true>(p.ctl, flags_x, NXT, seq, lane) : ps_wait_flags(p.ctl, flags_up, NHT, seq, lane);
        if (!alive) *s_dead = 1;
      }
      __syncthreads();
      f32x4 pa[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      if constexpr (top) {
        // gx_t [32 clips, fs] x W_p panel
        if (pw_on) {
          __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dxt) + (int64_t)t * BX, 0, (int)(BX * 4), 0x00020000);
          u32x4 a[2][NP];
#pragma unroll
          for (int u = 0; u < NP; ++u) {
            const unsigned ko = (unsigned)(((wid * NP + u) * 16 + 4 * g) * 4);
            a[0][u] = __builtin_amdgcn_raw_buffer_load_b128(xr, (unsigned)(ar0 * fs * 4) + ko, 0, 16);
            a[1][u] = __builtin_amdgcn_raw_buffer_load_b128(xr, (unsigned)(ar1 * fs * 4) + ko, 0, 16);
          }
          if (fs < FS) {     // k at or past fs: the load ran into the next clip's row (or past the buffer: zeros)
#pragma unroll
            for (int u = 0; u < NP; ++u)
              if (!pkv[u]) a[0][u] = a[1][u] = u32x4{0u, 0u, 0u, 0u};
          }
#pragma unroll
          for (int u = 0; u < NP; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int r = 0; r < 2; ++r)
                pa[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag_rbf_if(__uint_as_float(a[r][u][e]), RB), w2[u][e], pa[r], 0, 0, 0);
        }
      } else {
        // dg_{l+1,t} [32 clips, 4S] x W_ih_{l+1} panel: the register part, then the LDS part
        __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(dg_up + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
#pragma unroll
        for (int ub = 0; ub < NU; ub += UB) {
          u32x4 a[2][UB];
#pragma unroll
          for (int i = 0; i < UB; ++i) {
            a[0][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o0, (unsigned)((ub + i) * 64), 16);
            a[1][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o1, (unsigned)((ub + i) * 64), 16);
          }
#pragma unroll
          for (int i = 0; i < UB; ++i) {
            f32x4 wv;
            if (ub + i < NR2) {
#pragma unroll
              for (int e = 0; e < 4; ++e) wv[e] = w2[ub + i < NW2 ? ub + i : 0][e];
            } else {
              wv = *reinterpret_cast<const f32x4*>(&w2l[(wid * NL2 + (ub + i - NR2)) * 256 + lane * 4]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int r = 0; r < 2; ++r)
                pa[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag_rbf_if(__uint_as_float(a[r][i][e]), RB), wv[e], pa[r], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wid * 512 + (16 * r + 4 * g + e) * 16 + li] = pa[r][e];
      __syncthreads();
      if (epi) {
        float dhv = ext + carry;
#pragma unroll
        for (int w = 0; w < 8; ++w) dhv += red[w * 512 + tid];
        __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(dg_own + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
        const float tc = tanhf(cn);
        const float dc = dcn + dhv * og * (1.f - tc * tc);
        float d0 = dc * gg * ig * (1.f - ig);
        float d1 = dc * cp * fg * (1.f - fg);
        float d2 = dc * ig * (1.f - gg * gg);
        float d3 = dhv * tc * og * (1.f - og);
        dcn = dc * fg;
        if (*s_dead) { d0 = d1 = d2 = d3 = dcn = __builtin_nanf(""); }   // a wait timed out: poison instead of garbage
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d0), orr, og4, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d1), orr, og4 + (unsigned)(S * 4), 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d2), orr, og4 + (unsigned)(2 * S * 4), 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d3), orr, og4 + (unsigned)(3 * S * 4), 0, 16);
      }
    }
    if (t == 0 && !isx && l == 0) break;                      // dg_{0,0} has no reader inside the launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // EVERY storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
      __hip_atomic_store(my_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) break;
    // ---- the recurrent term of frame t-1: dg_{l,t} [32 clips, 4S] x the register panel
    if (wid == 0 && alive) {
      alive = ps_wait_flags(p.ctl, flags_own, NHT, seq, lane);
      if (!alive) *s_dead = 1;
    }
    __syncthreads();
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    {
      __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(dg_own + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
#pragma unroll
      for (int ub = 0; ub < NU; ub += UB) {
        u32x4 a[2][UB];
#pragma unroll
        for (int i = 0; i < UB; ++i) {
          a[0][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o0, (unsigned)((ub + i) * 64), 16);
          a[1][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o1, (unsigned)((ub + i) * 64), 16);
        }
#pragma unroll
        for (int i = 0; i < UB; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < 2; ++r)
              acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag_rbf_if(__uint_as_float(a[r][i][e]), RB), wreg[ub + i][e], acc[r], 0, 0, 0);
      }
    }
    // C layout of a 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + e
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wid * 512 + (16 * r + 4 * g + e) * 16 + li] = acc[r][e];
    __syncthreads();
    carry = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) carry += red[w * 512 + tid];
    __syncthreads();                                          // red is written again in the next frame
  }
}

template <int S, int FS, bool RB>
__global__ __launch_bounds__(512) void gfront_stack_bwd_kernel(const FrontStackBwdP p) {
  constexpr int NHT = S / 16, NU = 4 * S / 128, NL2 = FRONT_STACK_BWD_LDS_UNITS(NU);
  static_assert(NU * 128 == 4 * S && FS % 16 == 0 && FS / 16 <= 64 && S % 16 == 0, "shape");
  __shared__ float red[8 * 512];
  __shared__ __attribute__((aligned(16))) float w2l[NL2 > 0 ? 8 * NL2 * 256 : 4];      // [wave][k unit][g][li][e]
  __shared__ int s_dead;
  if (threadIdx.x == 0) s_dead = 0;
  __syncthreads();
  const int NT = p.nl * NHT + ((p.fs + 15) >> 4);           // tiles per clip tile
  const int bt = blockIdx.x / NT, ct = blockIdx.x % NT;
  if (ct >= p.nl * NHT) {
    front_stack_bwd_body<S, FS, RB, 0>(p, red, w2l, &s_dead, bt, ct, 0);      // (x tiles read layer 0's dgates)
  } else {
    const int l = ct / NHT;
    if (l == p.nl - 1) front_stack_bwd_body<S, FS, RB, 1>(p, red, w2l, &s_dead, bt, ct, l);
    else front_stack_bwd_body<S, FS, RB, 2>(p, red, w2l, &s_dead, bt, ct, l);
  }
}

// workgroups of the stacked backward: per clip tile nl * S/16 h tiles and ceil(fs/16) x tiles
static int64_t front_stack_bwd_grid(int B, int S, int fs, int nl) { return (int64_t)ag_cdiv(B, 32) * ((int64_t)nl * (S / 16) + ag_cdiv(fs, 16)); }

static bool front_stack_bwd_shape_ok(int B, int S, int fs, int nl, int n_cu) {
  if (nl < 2 || nl > FRONT_MAX_LAYERS) return false;
  if (!front_fs_ok(S, fs)) return false;
  if (B < 1) return false;
  if (n_cu > 256) n_cu = 256;
  const int64_t grid = front_stack_bwd_grid(B, S, fs, nl);
  return grid <= n_cu && grid <= (PS_HDR_BYTES / 4 - PS_FLAG_OFF);
}

extern "C" int ag_gfront_stack_bwd_ok(int B, int S, int fs, int nl, int n_cu) { return front_stack_bwd_shape_ok(B, S, fs, nl, n_cu) ? 1 : 0; }

extern "C" int64_t ag_gfront_stack_bwd_ws_bytes(int B, int S, int fs, int nl) {
  (void)B; (void)S; (void)fs; (void)nl;      // (dgs / dxt are the exchange buffers: the sticky word and the header only)
  return PS_STICKY_BYTES + PS_HDR_BYTES;
}

template <int S, int FS, bool RB>
static void front_stack_bwd_launch(const FrontStackBwdP& p, int grid, hipStream_t st) {
  static const AgKernelName name("gfront_stack_bwd_kernel", {S, FS, RB ? 1 : 0});
  ag_note_kernel(name.s);
  hipLaunchKernelGGL((gfront_stack_bwd_kernel<S, FS, RB>), dim3(grid), dim3(512), 0, st, p);
}

// The backward through time of a front with 2 to 8 LSTMCell layers in ONE launch.  Tensor contracts:
// ag_front_stack_bwd_args (include/audiogan_hip.h).  Shapes: ag_gfront_stack_bwd_ok.
extern "C" int ag_gfront_stack_bwd(const ag_front_stack_bwd_args* a, void* stream) {
  static const char* const who = "ag_gfront_stack_bwd";
  if (int rc = front_struct_ok(who, a, "ag_front_stack_bwd_args")) return rc;
  AG_REQUIRE(a->nl >= 1 && a->nl <= FRONT_MAX_LAYERS, "%s: nl = %d, the per-layer tables hold 1 to %d layers", who, a->nl, FRONT_MAX_LAYERS);
  const int nl = a->nl;
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    const FrontField f[] = {{"ga", a->ga[l], true}, {"cs", a->cs[l], true}, {"w_hh", a->w_hh[l], true}, {"w_in", a->w_in[l], true},
                            {"dgs", a->dgs[l], true}};
    if (int rc = front_layer_fields_ok(who, l, nl, f)) return rc;
  }
  const FrontField fields[] = {
      {"w_p", a->w_p, true}, {"x", a->x, true}, {"dh_ext", a->dh_ext, a->dh_ext != nullptr}, {"dx_ext", a->dx_ext, a->dx_ext != nullptr},      // (optional)
      {"dxt", a->dxt, true}, {"ws", a->ws, true}};
  if (int rc = front_fields_ok(who, fields)) return rc;
  const int T = a->T, B = a->B, S = a->S, fs = a->fs;
  AG_REQUIRE(T > 0, "%s: T must be positive", who);
  AG_REQUIRE(a->ldx >= (int64_t)T * fs, "%s: x row pitch smaller than a row", who);
  AG_REQUIRE(!a->dx_ext || a->lddx >= (int64_t)T * fs, "%s: dx_ext row pitch smaller than a row", who);
  AG_REQUIRE(a->ldwx >= fs, "%s: w_in[0] row pitch smaller than a row", who);
  if (!front_stack_bwd_shape_ok(B, S, fs, nl, a->n_cu)) {
    ag_set_error("%s: shape B=%d S=%d fs=%d nl=%d is not supported on %d CUs", who, B, S, fs, nl, a->n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  AG_REQUIRE((int64_t)B * 4 * S * 4 < ((int64_t)1 << 31), "%s: frame slab too large", who);
  uintptr_t al = (uintptr_t)a->dxt;
  for (int l = 0; l < nl; ++l) al |= (uintptr_t)a->dgs[l];
  AG_REQUIRE((al & 15) == 0, "%s: outputs must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  FrontStackBwdP p;
  if (int rc = persist_begin(who, a->ws, a->ws_bytes, ag_gfront_stack_bwd_ws_bytes(B, S, fs, nl), st, &p.ctl)) return rc;
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    p.ga[l] = a->ga[l]; p.cs[l] = a->cs[l]; p.whh[l] = a->w_hh[l]; p.win[l] = a->w_in[l]; p.dgs[l] = a->dgs[l];
  }
  p.wp = a->w_p; p.x = a->x; p.ldx = a->ldx; p.dh_ext = a->dh_ext; p.dx_ext = a->dx_ext; p.lddx = a->lddx; p.dxt = a->dxt;
  p.T = T; p.B = B; p.ldwx = a->ldwx; p.fs = fs; p.nl = nl;
  const bool rb = ag_precision() == AG_PREC_BF16;
  const int grid = (int)front_stack_bwd_grid(B, S, fs, nl);
  if (S == 1024) {
    if (rb) front_stack_bwd_launch<1024, 256, true>(p, grid, st);
    else front_stack_bwd_launch<1024, 256, false>(p, grid, st);
  } else {
    if (rb) front_stack_bwd_launch<128, 64, true>(p, grid, st);
    else front_stack_bwd_launch<128, 64, false>(p, grid, st);
  }
  AG_CHECK_LAUNCH(who);
  return AG_OK;
}

// front_persist.hip -- the one-layer generator front as ONE persistent launch per direction: gfront_persist_fwd_kernel
// (LSTM and GRU cell, bf16 MFMAs, generation mode) and gfront_persist_bwd_kernel.  The hand-off protocol is that of the layer
// kernels (lstm_persist.hip, persist_common.h); the blocks of the frame loops shared with the stacked front
// (front_stack.hip) are in front_parts.h.
#include "front_parts.h"

#include <type_traits>

// ------------------------------------------------------------------------------------------
// The Generator's recurrent front (audiogan.py:428-460, one LSTMCell layer) as ONE persistent launch:
//   frame t:  gates = pre_t + [x_{t-1} | h_{t-1}] [W_x | W_hh]^T ;  (c_t, h_t) = cell(gates) ;  x_t = tanh(h_t W_p^T + b_p)
// (pre_t = the z/c columns of W_ih and both biases, one GEMM over all frames beforehand; the stop head is one GEMM over
// all frames afterwards).  Per frame the launch-per-op path costs a fused step kernel plus a projection kernel, each
// re-streaming its weights (21 MB + 1 MB); here every weight stays in REGISTERS for all T frames:
//
//   workgroup (rt, ut): 32 clips x 8 hidden units (32 gate columns); its 8 waves split K: each holds S/8 rows of the
//   [W_hh] panel and fs/8 rows of the [W_x] panel as MFMA B operands (80 VGPRs at S = 1024, fs = 256).
//   phase A, frame t: h_{t-1} part of the product as soon as the group's h flags are up, x_{t-1} part when the
//   projection tiles are up, LDS sum over the waves, cell, h_t published (write-through) + flag.
//   phase B, frame t (workgroups ut < 2*ceil(fs/16) only): one [16 clips x 16 frame samples] tile of x_t = tanh(h_t W_p^T + b):
//   waits for all h_t of its clips, v_mfma_f32_16x16x4_f32 against its resident W_p panel, publishes x_t + flag.
//   The h part of frame t+1 (80 % of the MFMAs) overlaps phase B of frame t on the other workgroups.
// Exchange buffers ([parity][rt][8-unit tile][32 clips][8], as in the layer kernels) hold h and x; two parities are
// enough (h_{t+1} / x_{t+1} are written only after every reader of h_{t-1} / x_{t-1} has finished frame t).
//
// Frame sizes below the panel width: the template parameter FS is the PADDED width of the x panel (256 at S = 1024, 64 at
// S = 128), the real frame size p.fs (a multiple of 8, <= FS) is a run-time field.  k lanes of the W_x panel at or past fs
// hold zeros (masked, not loaded: to the right of column fs in a row of W_ih lie the z/c weights), the 2 * ceil(fs / 16)
// projection workgroups take rows of W_p / b_p past fs as zeros, the 8-column groups of the x exchange buffer past fs are
// zeroed once by the projection workgroups before their first flag, and every global row uses fs as its pitch.  At
// fs == FS nothing is masked and the arithmetic and its order are those of the fixed-width form.
// ------------------------------------------------------------------------------------------
struct FrontFwdP {
  float* gates;        // [T,B,4S] in: pre; out: activated gates
  const float* wx;     // W_ih[:, :fs]   [4S, ldwx]
  const float* whh;    // [4S, S]
  const float* wp;     // [fs, S]
  const float* bp;     // [fs]
  float* hs;           // [T,B,S]
  float* cs;           // [T+1,B,S]  (cs[0] is written 0 by the launch)
  float* x;            // [B, T*fs], row pitch ldx (the caller may hand over channel 0 of the conv trunk's slab)
  float* xt;           // optional [T,B,fs]: the same frames time-major (what the weight-gradient products read)
  int64_t ldx;
  float* gh;           // GRU cell only: [T,B,3S], the n slot receives W_hn h + b_hn (what the backward needs)
  const float* bhn;    // GRU cell only: b_hh[2S:3S]
  float* hx;           // exchange: h   [2][nrt][S/8][32][8]
  float* xx;           // exchange: x   [2][nrt][FS/8][32][8]  (FS = the padded panel width)
  PersistCtl ctl;
  int T, B, ldwx, nrt, rb;
  int fs;              // the real frame size: fs % 8 == 0, 8 <= fs <= FS
};

// (generation mode: the rule and its header words are described in front_parts.h)
struct FrontGenP : FrontFwdP {
  const float* ws;     // stop head: materialised weight [S], bias [1]
  const float* bs;
  const float* u;      // [T,B] uniforms
  float* s;            // [B,T] out, row pitch lds: stop logits of the frames run
  int64_t lds;
  int* first;          // [B] out: frames generated per clip (1 + first stop frame, T if none)
  int* t_run;          // [1] out: frames run
};

// PM: 0 = as stored / operands rounded in registers when p.rb (fp32 MFMA); 2 = AG_PREC_BF16 on the bf16 MFMAs (panels
// in registers as bf16: 8 k per 4 VGPRs)
// CELL: 0 = LSTMCell (4 gate columns per unit: i f g o).  1 = GRU cell (BASELINE configs[3]; PM = 0 only): the 4 column
// blocks of a unit tile are  r | z | n_h | n_x : the h panel carries W_hr, W_hz, W_hn and zeros, the x panel W_xr, W_xz,
// zeros and W_xn, so that ONE accumulator ends up with  r, z pre-activations complete and the two halves of n apart
// (n = tanh(n_x + r * (n_h + b_hn)));  h_t = (1 - z) n + z h_{t-1} stays in a register like the LSTM's cell state.
// GEN: 1 = generation mode (FrontGenP, see above); 0 = the training forward.
template <int S, int FS, int PM, int CELL = 0, int GEN = 0>
__global__ __launch_bounds__(512) void gfront_persist_fwd_kernel(const typename std::conditional<GEN == 1, FrontGenP, FrontFwdP>::type p) {
  constexpr int NUT = S / 8;                 // unit tiles = workgroups per row tile
  constexpr int QH = S / 64, QX = FS / 64;   // 8-k groups of the h / x panel per wave
  constexpr int NBMAX = 2 * (FS / 16);       // projection tiles per row tile at fs == FS (2 x 16-clip subtiles)
  constexpr int UP = S / 128;                // 16-k units of W_p per wave
  static_assert(S % 128 == 0 && FS % 64 == 0 && NBMAX <= NUT && NBMAX <= 64, "unsupported front shape");
  __shared__ float red[8 * 1024];
  __shared__ int s_dead;
  __shared__ int s_exit;       // (generation mode) the loop ends here
  const int T = p.T, B = p.B, fs = p.fs;
  const int NB = 2 * ((fs + 15) >> 4);       // projection tiles per row tile (the last column tile is half valid at fs % 16 == 8)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5, li = lane & 15, g = lane >> 4;
  if (tid == 0) s_dead = 0;
  __syncthreads();
  const int rt = blockIdx.x % p.nrt, ut = blockIdx.x / p.nrt;
  const int u0 = ut * 8, row0 = rt * 32;

  // ---- resident panels (B operands).  Gate column j = gate (j>>3), unit u0 + (j&7).
  constexpr int QHf = PM == 2 ? 1 : QH, QXf = PM == 2 ? 1 : QX, QH2 = PM == 2 ? QH / 2 : 1, QX2 = PM == 2 ? QX / 2 : 1;
  float wh[QHf][4], wxr[QXf][4];
  ps_bf16x8 whb[QH2], wxb[QX2];
  if (PM == 2) {
    const int wrow = (l31 >> 3) * S + u0 + (l31 & 7);
#pragma unroll
    for (int Q = 0; Q < QH2; ++Q) {
      const float* src = p.whh + (int64_t)wrow * S + (wid * QH + 2 * Q + hh) * 8;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
      ps_u32x4 r = {ag_pack_bf16(a[0], a[1]), ag_pack_bf16(a[2], a[3]), ag_pack_bf16(b[0], b[1]), ag_pack_bf16(b[2], b[3])};
      whb[Q] = __builtin_bit_cast(ps_bf16x8, r);
    }
#pragma unroll
    for (int Q = 0; Q < QX2; ++Q) {
      const int kx = (wid * QX + 2 * Q + hh) * 8;
      ps_u32x4 r = {0u, 0u, 0u, 0u};
      if (kx < fs) {          // (k >= fs: zeros - what lies there in the row are the z/c weights)
        const float* src = p.wx + (int64_t)wrow * p.ldwx + kx;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
        r = ps_u32x4{ag_pack_bf16(a[0], a[1]), ag_pack_bf16(a[2], a[3]), ag_pack_bf16(b[0], b[1]), ag_pack_bf16(b[2], b[3])};
      }
      wxb[Q] = __builtin_bit_cast(ps_bf16x8, r);
    }
  } else {
    const int cb = l31 >> 3;
    // (GRU: column block 3 of the h panel and block 2 of the x panel are zero; block 3 of the x panel is W_xn)
    const bool hz = CELL == 1 && cb == 3, xz = CELL == 1 && cb == 2;
    const int wrow = cb * S + u0 + (l31 & 7), wrowx = (CELL == 1 && cb == 3 ? 2 : cb) * S + u0 + (l31 & 7);
#pragma unroll
    for (int q = 0; q < QH; ++q) {
      const f32x4 v = hz ? f32x4{0.f, 0.f, 0.f, 0.f}
                         : ag_rbf4_if(*reinterpret_cast<const f32x4*>(p.whh + (int64_t)wrow * S + (wid * QH + q) * 8 + 4 * hh), p.rb);
#pragma unroll
      for (int e = 0; e < 4; ++e) wh[q][e] = v[e];
    }
#pragma unroll
    for (int q = 0; q < QX; ++q) {
      const int kx = (wid * QX + q) * 8 + 4 * hh;       // (k >= fs: zeros - what lies there in the row are the z/c weights)
      const f32x4 v = (xz || kx >= fs) ? f32x4{0.f, 0.f, 0.f, 0.f}
                                       : ag_rbf4_if(*reinterpret_cast<const f32x4*>(p.wx + (int64_t)wrowx * p.ldwx + kx), p.rb);
#pragma unroll
      for (int e = 0; e < 4; ++e) wxr[q][e] = v[e];
    }
  }
  const bool bwg = ut < NB;                  // this workgroup also owns a projection tile
  const int bsub = ut & 1, bcol0 = (ut >> 1) * 16;
  const bool wpv = bwg && bcol0 + li < fs;   // this lane's row of W_p exists (rows past fs read as zeros)
  constexpr int UPf = PM == 2 ? 1 : UP, UP2 = PM == 2 ? UP / 2 : 1;
  float wpr[UPf][4];
  ps_bf16x8b wpb[UP2];
  if (PM == 2) {
#pragma unroll
    for (int U = 0; U < UP2; ++U) {
      ps_u32x4 r = {0u, 0u, 0u, 0u};
      if (wpv) {
        const float* src = p.wp + (int64_t)(bcol0 + li) * S + (wid * UP2 + U) * 32 + 8 * g;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
        r = ps_u32x4{ag_pack_bf16(a[0], a[1]), ag_pack_bf16(a[2], a[3]), ag_pack_bf16(b[0], b[1]), ag_pack_bf16(b[2], b[3])};
      }
      wpb[U] = __builtin_bit_cast(ps_bf16x8b, r);
    }
  } else {
#pragma unroll
    for (int u = 0; u < UPf; ++u) {
      const f32x4 v = wpv ? ag_rbf4_if(*reinterpret_cast<const f32x4*>(p.wp + (int64_t)(bcol0 + li) * S + (wid * UP + u) * 16 + 4 * g), p.rb)
                          : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) wpr[u][e] = v[e];
    }
  }
  // generation mode: the stop head's weight in LDS, on the stop workgroups only.  (Not in registers: the fp32 form at S = 1024
  // holds 243 VGPRs already and would spill; a lane reads its 4 / 8 contiguous k per 16-k unit with one / two ds_read_b128.)
  const bool swg = GEN == 1 && ut < 2;
  __shared__ __attribute__((aligned(16))) float wsl[GEN == 1 ? S : 4];
  float bsv = 0.f;
  if constexpr (GEN == 1) {
    if (swg) {
      for (int k = tid; k < S; k += 512) wsl[k] = p.ws[k];
      bsv = p.bs[0];
    }
    __syncthreads();
  }

  unsigned* flag_h = p.ctl.hdr + PS_FLAG_OFF + rt * NUT;
  unsigned* flag_x = p.ctl.hdr + PS_FLAG_OFF + p.nrt * NUT + rt * NB;
  const int64_t hgs = (int64_t)NUT * 32 * 8, xgs = (int64_t)(FS / 8) * 32 * 8;     // floats per (parity, rt)
  __amdgpu_buffer_rsrc_t hr = __builtin_amdgcn_make_buffer_rsrc(p.hx, 0, (int)(2 * p.nrt * hgs * 4), 0x00020000);
  __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(p.xx, 0, (int)(2 * p.nrt * xgs * 4), 0x00020000);

  // phase A epilogue role: thread (clip row, unit), tid < 256
  const int erow = tid >> 3, euu = tid & 7;
  const int em = row0 + erow, eu = u0 + euu;
  const bool epi = tid < 256 && em < B;
  const int ee = (erow & 3) + 4 * (erow >> 3), ehq = (erow >> 2) & 1;
  float creg = 0.f;            // LSTM: cell state; GRU: h_{t-1}
  const float ebhn = (CELL == 1 && epi) ? p.bhn[eu] : 0.f;
  // phase B epilogue role: thread (clip row within the 16-row subtile, column), tid < 256
  const int brow = tid >> 4, bcl = tid & 15;
  const int bm = row0 + 16 * bsub + brow;
  const bool bcv = bcol0 + bcl < fs;         // this thread's frame sample exists
  const float bbias = (bwg && tid < 256 && bcv) ? p.bp[bcol0 + bcl] : 0.f;
  bool alive = true;
  // fs < FS: the 8-column groups of the x exchange buffer from roundup(fs, 16) / 8 on have no owner; the projection workgroups
  // share them out and write zeros into both parities once.  Every wave drains its stores before the barrier in front of the
  // workgroup's first x flag, and a reader of x waits for all NB flags, so the zeros are in place before the first read.
  if (bwg && tid < 256) {
    for (int gp = NB + ut; gp < FS / 8; gp += NB) {
#pragma unroll
      for (int par = 0; par < 2; ++par)
        __builtin_amdgcn_raw_buffer_store_b32(0u, xr, (unsigned)(((int64_t)(par * p.nrt + rt) * xgs + (int64_t)gp * 256 + tid) * 4), 0, 16);
    }
  }

  // (the pre-activations of frame t + 1 are requested at the end of frame t, after the flag and before the trailing stores, and
  // nothing is written at the top of the loop - as in lstm_persist_fwd_kernel, where the re-initialisation of these registers made
  // every step begin with a wait for the previous step's trailing stores)
  float pre4[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_pre = [&](int tt) {
    if (epi) {
      if (CELL == 1) {
        const float* pr = p.gates + ((int64_t)tt * B + em) * 3 * S + eu;
        pre4[0] = pr[0]; pre4[1] = pr[S]; pre4[2] = pr[2 * S];
      } else {
        const float* pr = p.gates + ((int64_t)tt * B + em) * 4 * S + eu;
        pre4[0] = pr[0]; pre4[1] = pr[S]; pre4[2] = pr[2 * S]; pre4[3] = pr[3 * S];
      }
    }
  };
  load_pre(0);
  // generation mode: thread tid < 16 of a stop workgroup owns clip sm of its subtile (first stop, next uniform)
  const int nsub = 2 * p.nrt, sub = 2 * rt + (ut & 1);
  unsigned* gen_done = p.ctl.hdr + PS_GEN_OFF;
  unsigned* gen_all = gen_done + 8;
  const int sm = row0 + 16 * (ut & 1) + tid;
  const bool sthr = swg && tid < 16 && sm < B;
  int fst = T, t_ran = T;
  bool all_pub = false;
  float ureg = 1.f;
  if constexpr (GEN == 1) {
    if (sthr) ureg = p.u[sm];
  }
  for (int t = 0; t < T; ++t) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (t > 0) {
      const int par = (t - 1) & 1;
      // ---- h part (its flags were already waited for by the projection phase of frame t-1 on projection workgroups)
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
      if (wid == 0 && alive && !ex) {
        alive = ps_wait_flags(p.ctl, flag_h, NUT, (unsigned)t, lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      if constexpr (GEN == 1) {
        if (s_exit) { t_ran = t; break; }
      }
      if (PM == 2) {
        const unsigned ab = (unsigned)(((int64_t)(par * p.nrt + rt) * hgs + (int64_t)l31 * 8) * 4);
        u32x4 a0[QH2], a1[QH2];
#pragma unroll
        for (int Q = 0; Q < QH2; ++Q) {
          const unsigned o = ab + (unsigned)((wid * QH + 2 * Q + hh) * 32 * 32);
          a0[Q] = __builtin_amdgcn_raw_buffer_load_b128(hr, o, 0, 16);
          a1[Q] = __builtin_amdgcn_raw_buffer_load_b128(hr, o + 16u, 0, 16);
        }
#pragma unroll
        for (int Q = 0; Q < QH2; ++Q) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ps_pack8(a0[Q], a1[Q]), whb[Q], acc, 0, 0, 0);
      } else {
        const unsigned ab = (unsigned)(((int64_t)(par * p.nrt + rt) * hgs + (int64_t)l31 * 8 + 4 * hh) * 4);
        u32x4 a[QH];
#pragma unroll
        for (int q = 0; q < QH; ++q) a[q] = __builtin_amdgcn_raw_buffer_load_b128(hr, ab + (unsigned)((wid * QH + q) * 32 * 32), 0, 16);
        if (p.rb) {
#pragma unroll
          for (int q = 0; q < QH; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[q][e] = __float_as_uint(ag_rbf(__uint_as_float(a[q][e])));
        }
#pragma unroll
        for (int q = 0; q < QH; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[q][e]), wh[PM == 2 ? 0 : q][e], acc, 0, 0, 0);
      }
      // ---- x part
      if (wid == 0 && alive) {
        alive = ps_wait_flags<true>(p.ctl, flag_x, NB, (unsigned)t, lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      if (PM == 2) {
        const unsigned ab = (unsigned)(((int64_t)(par * p.nrt + rt) * xgs + (int64_t)l31 * 8) * 4);
        u32x4 a0[QX2], a1[QX2];
#pragma unroll
        for (int Q = 0; Q < QX2; ++Q) {
          const unsigned o = ab + (unsigned)((wid * QX + 2 * Q + hh) * 32 * 32);
          a0[Q] = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 16);
          a1[Q] = __builtin_amdgcn_raw_buffer_load_b128(xr, o + 16u, 0, 16);
        }
#pragma unroll
        for (int Q = 0; Q < QX2; ++Q) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ps_pack8(a0[Q], a1[Q]), wxb[Q], acc, 0, 0, 0);
      } else {
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
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[q][e]), wxr[PM == 2 ? 0 : q][e], acc, 0, 0, 0);
      }
    }
    front_acc_to_red(red, wid, lane, acc);
    __syncthreads();
    float hreg = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f;
    if (epi) {
      float g4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float s = CELL == 1 ? 0.f : pre4[q];
        if (t > 0) {
#pragma unroll
          for (int w = 0; w < 8; ++w) s += red[w * 1024 + ee * 64 + 32 * ehq + 8 * q + euu];
        }
        g4[q] = s;
      }
      if (CELL == 1) {
        // ig / fg / gg = r / z / n;  og = the h half of n incl. its bias (saved for the backward)
        og = g4[2] + ebhn;
        ig = ag_sigmoid(pre4[0] + g4[0]); fg = ag_sigmoid(pre4[1] + g4[1]); gg = tanhf(pre4[2] + g4[3] + ig * og);
        hreg = (1.f - fg) * gg + fg * creg;
        creg = hreg;
      } else {
        ig = ag_sigmoid(g4[0]); fg = ag_sigmoid(g4[1]); gg = tanhf(g4[2]); og = ag_sigmoid(g4[3]);
        creg = fg * creg + ig * gg;
        hreg = og * tanhf(creg);
      }
      if (s_dead) creg = hreg = ig = __builtin_nanf("");             // a wait timed out: poison instead of garbage
    }
    if (tid < 256) {
      // publish h_t (rows past the batch: zeros, so that the exchange buffer stays defined)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hreg), hr,
          (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + ((int64_t)ut * 32 + erow) * 8 + euu) * 4), 0, 16);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
      __hip_atomic_store(flag_h + ut, (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // this frame's pre-activations were consumed above (ig .. og hold what goes back into their place)
    if (t + 1 < T) load_pre(t + 1);
    if (GEN == 0 && epi) {      // (the generation mode keeps no history)
      if (CELL == 1) {
        float* pr = p.gates + ((int64_t)t * B + em) * 3 * S + eu;
        pr[0] = ig; pr[S] = fg; pr[2 * S] = gg;
        p.gh[((int64_t)t * B + em) * 3 * S + 2 * S + eu] = og;
      } else {
        float* pr = p.gates + ((int64_t)t * B + em) * 4 * S + eu;
        pr[0] = ig; pr[S] = fg; pr[2 * S] = gg; pr[3 * S] = og;
        if (t == 0) p.cs[(int64_t)em * S + eu] = 0.f;               // c_0 = 0: written here, so the caller need not fill it
        p.cs[((int64_t)(t + 1) * B + em) * S + eu] = creg;
      }
      p.hs[((int64_t)t * B + em) * S + eu] = hreg;
    }
    // ---- phase B: this workgroup's tile of x_t = tanh(h_t W_p^T + b)
    if (bwg) {
      if (wid == 0 && alive) {
        alive = ps_wait_flags(p.ctl, flag_h, NUT, (unsigned)(t + 1), lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      f32x4 pacc = {0.f, 0.f, 0.f, 0.f};
      float sdot = 0.f;          // (generation mode, stop workgroups) this lane's part of h_t . w_s
      if (PM == 2) {
        // lane (clip li, k slot g) takes k = 32U + 8g .. +7 = the whole row of unit tile 4U + g
        const unsigned ab = (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + (int64_t)(16 * bsub + li) * 8) * 4);
        u32x4 a0[UP2], a1[UP2];
#pragma unroll
        for (int U = 0; U < UP2; ++U) {
          const unsigned o = ab + (unsigned)((4 * (wid * UP2 + U) + g) * 32 * 32);
          a0[U] = __builtin_amdgcn_raw_buffer_load_b128(hr, o, 0, 16);
          a1[U] = __builtin_amdgcn_raw_buffer_load_b128(hr, o + 16u, 0, 16);
        }
#pragma unroll
        for (int U = 0; U < UP2; ++U)
          pacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ps_bf16x8b, ps_pack8(a0[U], a1[U])), wpb[U], pacc, 0, 0, 0);
        if constexpr (GEN == 1) {
          if (swg) {     // (the stop logit from the unrounded h_t)
#pragma unroll
            for (int U = 0; U < UP2; ++U) {
              const float* wk = wsl + 32 * (wid * UP2 + U) + 8 * g;
              const f32x4 w0 = *reinterpret_cast<const f32x4*>(wk), w1 = *reinterpret_cast<const f32x4*>(wk + 4);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                sdot = fmaf(__uint_as_float(a0[U][j]), w0[j], sdot);
                sdot = fmaf(__uint_as_float(a1[U][j]), w1[j], sdot);
              }
            }
          }
        }
      } else {
        // A = h_t rows of the 16-clip subtile: lane (clip li, k slot g) takes k = 16u + 4g .. +3 = unit tile 2u + (g>>1), half g&1
        const unsigned ab = (unsigned)(((int64_t)((t & 1) * p.nrt + rt) * hgs + (int64_t)(16 * bsub + li) * 8 + 4 * (g & 1)) * 4);
        u32x4 a[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u)
          a[u] = __builtin_amdgcn_raw_buffer_load_b128(hr, ab + (unsigned)((2 * (wid * UP + u) + (g >> 1)) * 32 * 32), 0, 16);
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
          for (int e = 0; e < 4; ++e) pacc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[u][e]), wpr[PM == 2 ? 0 : u][e], pacc, 0, 0, 0);
      }
      // 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + e   (red is free again: the gate sums were consumed above)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wid * 256 + (4 * g + e) * 16 + li] = pacc[e];
      if constexpr (GEN == 1) {
        if (swg) {       // the 4 k slots of a clip, then (below) the 8 waves: the same LDS pass as pacc
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
            if (sthr && t + 1 < T) ureg = p.u[(int64_t)(t + 1) * B + sm];
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
static bool front_shape_ok(int B, int S, int fs, int n_cu) {
  if (!front_fs_ok(S, fs)) return false;
  if (B < 1 || B > 64) return false;
  if (n_cu > 256) n_cu = 256;
  return ag_cdiv(B, 32) * (S / 8) <= n_cu;
}

extern "C" int ag_gfront_persist_ok(int B, int S, int fs, int n_cu) { return front_shape_ok(B, S, fs, n_cu) ? 1 : 0; }

extern "C" int64_t ag_gfront_persist_ws_bytes(int B, int S, int fs) {
  // (the x exchange buffer has the padded panel width whatever fs is; shapes outside the set: the formula of the exact width)
  const int w = front_fs_ok(S, fs) ? front_panel(S) : fs;
  return PS_STICKY_BYTES + PS_HDR_BYTES + (int64_t)2 * ag_cdiv(B, 32) * 32 * (S + w) * 4;
}
// The frame loop of the Generator front in ONE launch: training forward and generation mode, LSTM and GRU cell.  Tensor
// contracts: ag_front_fwd_args (include/audiogan_hip.h).  Shapes: ag_gfront_persist_ok.
extern "C" int ag_gfront_fwd(const ag_front_fwd_args* a, void* stream) {
  static const char* const who = "ag_gfront_fwd";
  if (int rc = front_struct_ok(who, a, "ag_front_fwd_args")) return rc;
  AG_REQUIRE((a->cell == 0 || a->cell == 1) && (a->gen == 0 || a->gen == 1),
             "%s: cell must be 0 (LSTM) or 1 (GRU) and gen 0 (training) or 1 (generation)", who);
  const bool gru = a->cell == 1, gen = a->gen == 1;
  const FrontField fields[] = {
      {"gates", a->gates, true}, {"gh", a->gh, gru && !gen}, {"w_x", a->w_x, true}, {"w_hh", a->w_hh, true},
      {"b_hn", a->b_hn, gru}, {"w_p", a->w_p, true}, {"b_p", a->b_p, true}, {"hs", a->hs, !gen}, {"cs", a->cs, !gru && !gen},
      {"x", a->x, true}, {"xt", a->xt, !gen && a->xt},      // (optional in training)
      {"w_s", a->w_s, gen}, {"b_s", a->b_s, gen}, {"u", a->u, gen}, {"s", a->s, gen}, {"first", a->first, gen},
      {"t_run", a->t_run, gen}, {"ws", a->ws, true}};
  if (int rc = front_fields_ok(who, fields)) return rc;
  const int T = a->T, B = a->B, S = a->S, fs = a->fs;
  AG_REQUIRE(T > 0, "%s: T must be positive", who);
  AG_REQUIRE(a->ldx >= (int64_t)T * fs, "%s: x row pitch smaller than a row", who);
  AG_REQUIRE(!gen || a->lds >= T, "%s: s row pitch smaller than a row", who);
  if (!front_shape_ok(B, S, fs, a->n_cu)) {
    ag_set_error("%s: shape B=%d S=%d fs=%d is not supported on %d CUs", who, B, S, fs, a->n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  AG_REQUIRE(a->ldwx >= fs && a->ldwx % 4 == 0 && (((uintptr_t)a->w_x | (uintptr_t)a->w_hh | (uintptr_t)a->w_p) & 15) == 0,
             "%s: weights must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  FrontGenP p;      // (the training kernels take its base part, FrontFwdP)
  if (int rc = persist_begin(who, a->ws, a->ws_bytes, ag_gfront_persist_ws_bytes(B, S, fs), st, &p.ctl)) return rc;
  p.gates = a->gates; p.gh = a->gh; p.bhn = a->b_hn; p.wx = a->w_x; p.whh = a->w_hh; p.wp = a->w_p; p.bp = a->b_p;
  p.hs = a->hs; p.cs = a->cs; p.x = a->x; p.ldx = a->ldx; p.xt = a->xt;
  p.ws = a->w_s; p.bs = a->b_s; p.u = a->u; p.s = a->s; p.lds = a->lds; p.first = a->first; p.t_run = a->t_run;
  p.nrt = ag_cdiv(B, 32);
  p.hx = (float*)((char*)a->ws + PS_STICKY_BYTES + PS_HDR_BYTES);
  p.xx = p.hx + (int64_t)2 * p.nrt * 32 * S;
  p.T = T; p.B = B; p.ldwx = a->ldwx; p.fs = fs; p.rb = ag_precision() == AG_PREC_BF16;
  const int grid = p.nrt * (S / 8);
  // (the GRU front and S = 128 have no bf16-MFMA form)
  if (!gen) {
    void (*kern)(const FrontFwdP) =
        !gru ? (S == 1024 ? (p.rb ? gfront_persist_fwd_kernel<1024, 256, 2> : gfront_persist_fwd_kernel<1024, 256, 0>)
                          : gfront_persist_fwd_kernel<128, 64, 0>)
             : (S == 1024 ? gfront_persist_fwd_kernel<1024, 256, 0, 1> : gfront_persist_fwd_kernel<128, 64, 0, 1>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, static_cast<const FrontFwdP&>(p));
  } else {
    void (*kern)(const FrontGenP);
    if (S == 1024 && gru) kern = gfront_persist_fwd_kernel<1024, 256, 0, 1, 1>;
    else if (S == 1024) kern = p.rb ? gfront_persist_fwd_kernel<1024, 256, 2, 0, 1> : gfront_persist_fwd_kernel<1024, 256, 0, 0, 1>;
    else kern = gru ? gfront_persist_fwd_kernel<128, 64, 0, 1, 1> : gfront_persist_fwd_kernel<128, 64, 0, 0, 1>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, p);
  }
  AG_CHECK_LAUNCH(who);
  return AG_OK;
}
// ------------------------------------------------------------------------------------------
// Backward through time of the Generator's recurrent front (audiogan.py:428-460 under .backward() :903) as ONE
// persistent launch.  Per frame t (T-1 .. 0), with dacc[t] = [dL/dh_t | dL/dx_t] (the stop head's and the conv trunk's
// gradients, filled in by the host) as the external part:
//   gx_t  = (dacc_x[t] + dgates_{t+1} W_x) * (1 - x_t^2)                       d(pre-tanh) of the projection
//   dh_t  = dacc_h[t] + dgates_{t+1} W_hh + gx_t W_p
//   dgates_t = cell backward(dh_t, dc_{t+1})
// The launch-per-op path costs three launches per frame (fused cell step, a [B,4S] x [4S,S+fs] product that re-streams
// its 21 MB of weights from the fabric, the second stage of its K split).  Here every weight stays in REGISTERS:
//   workgroup (clip tile of 32, column tile of 16): one 16-column tile of [W_hh | W_x] = a [4S x 16] panel, K split
//   over the 8 waves (128 VGPRs per lane at S = 1024); S/16 "h tiles" + fs/16 "x tiles" per clip tile.
//   x tile, frame t: dx_t -> gx_t, published (write-through into dxt[t], which is also an output) + flag
//   h tile, frame t: waits for gx_t -> gx_t W_p against its resident [fs x 16] W_p panel -> cell backward of its
//                    (clip, unit) pairs (dc stays in a register) -> dgates_t published (into dgs[t]) + flag
//   both, t > 0    : wait for all dgates_t of the clip tile -> [32 x 4S] x panel on v_mfma_f32_16x16x4_f32 -> LDS sum of
//                    the 8 K slices -> the recurrent term of frame t-1, kept in a register.
// Two hand-offs per frame; one slot per frame in dgs / dxt (no parity); flags count frames.
// Frame sizes below the panel width (fs % 8 == 0, fs <= FS, as in the forward): ceil(fs / 16) x tiles per clip tile, so the
// grid is ceil(B/32) * (S/16 + ceil(fs/16)); columns at or past fs of the last x tile hold a zero W_x panel and neither load
// nor store anything; the k lanes of the projection product at or past fs hold zeros on both sides; fs is the row pitch of
// x, dx_ext and dxt.
// ------------------------------------------------------------------------------------------
struct FrontBwdP {
  const float* ga;     // [T,B,4S] activated gates (i, f, g, o)
  const float* c_all;  // [T+1,B,S]
  const float* x;      // [B,T*fs] the front's output (after tanh), row pitch ldx
  const float* dh_ext; // [T,B,S] external gradient dL/dh_t (the stop head's), or NULL = none
  const float* dx_ext; // [B,T*fs] external gradient dL/dx_t (the conv trunk's), row pitch lddx, or NULL = none
  int64_t ldx, lddx;
  const float* w_hh;   // [4S,S]
  const float* w_x;    // [4S,ldwx]: W_ih[:, :fs]
  const float* w_p;    // [fs,S]
  float* dgs;          // [T,B,4S] out (and exchange)
  float* dxt;          // [T,B,fs] out (and exchange)
  // GRU cell (CELL = 1): ga = activated (r, z, n) [T,B,3S], c_all = hs [T+1,B,S] (hs[t] = h_{t-1}), gh [T,B,3S] (its n
  // slot: W_hn h_{t-1} + b_hn); dgs = dgi [T,B,3S] (what the x tiles multiply by W_x), dgh [T,B,3S] (what the h tiles
  // multiply by W_hh: the n slot times r).  LSTM: gh unused, dgh = dgs.
  const float* gh;
  float* dgh;
  PersistCtl ctl;
  int T, B, ldwx;
  int fs;              // the real frame size: fs % 8 == 0, 8 <= fs <= FS
};

template <int S, int FS, bool RB, int CELL = 0>
__global__ __launch_bounds__(512) void gfront_persist_bwd_kernel(const FrontBwdP p) {
  constexpr int NG = CELL == 1 ? 3 : 4;                     // gate blocks
  constexpr int K4 = NG * S, NU = K4 / 128;                 // 16-k units of the big product per wave
  constexpr int NHT = S / 16;
  constexpr int NP = FS >= 128 ? FS / 128 : 1;              // 16-k units of the projection product per wave
  static_assert(NU * 128 == K4 && FS % 16 == 0 && FS / 16 <= 64 && S % 16 == 0, "shape");
  __shared__ float red[8 * 512];
  __shared__ int s_dead;
  const int T = p.T, B = p.B, fs = p.fs;
  const int NXT = (fs + 15) >> 4, NT = NHT + NXT;           // x tiles / all tiles per clip tile
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  if (tid == 0) s_dead = 0;
  __syncthreads();
  // placement: workgroup ids go round-robin over the 8 XCDs; with nbt clip tiles (8 % nbt == 0) a clip tile's NT workgroups
  // are put on 8 / nbt XCDs, so a frame's dgates rows are pulled into that many L2s instead of all 8 (speed only)
  int bt = blockIdx.x / NT, ct = blockIdx.x % NT;
  {
    const int nbt = gridDim.x / NT, per = nbt <= 8 ? 8 / nbt : 0;
    if (per > 0 && per * nbt == 8 && NT % per == 0) {
      const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;       // q < NT / per
      bt = xcd / per;
      ct = (xcd % per) * (NT / per) + q;
    } else if (per > 0 && per * nbt == 8) {
      // NT not a multiple of `per` (frame sizes below the panel width, e.g. 77 tiles at fs = 200): the XCD groups do not
      // hold NT workgroups each.  Slot l of group g takes tile l of clip tile g; the few slots past NT of the larger groups
      // take, in order, the tiles the smaller groups have no slot for.  A bijection for every grid; all but those few
      // workgroups of a clip tile still share 8 / nbt XCDs.
      const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
      const int full = gridDim.x >> 3, rem = gridDim.x & 7;
      auto cap = [&](int gq) { return per * full + min(max(rem - gq * per, 0), per); };   // workgroups on the XCDs of group gq
      const int gq = xcd / per, l = (xcd % per) + per * q;
      if (l < NT) {
        bt = gq; ct = l;
      } else {
        int r = l - NT;
        for (int g2 = 0; g2 < gq; ++g2) r += max(cap(g2) - NT, 0);
        for (int g2 = 0; g2 < nbt; ++g2) {
          const int miss = max(NT - cap(g2), 0);
          if (r < miss) { bt = g2; ct = cap(g2) + r; break; }
          r -= miss;
        }
      }
    }
  }
  const bool isx = ct >= NHT;
  const int m0 = bt * 32;
  const int n0 = (isx ? ct - NHT : ct) * 16;                // first column inside W_hh / W_x
  const int64_t BG = (int64_t)B * K4, BH = (int64_t)B * S, BX = (int64_t)B * fs;

  // resident panel: wreg[u][e] = W[(wid*NU + u)*16 + 4g + e][n0 + li]
  float wreg[NU][4];
  {
    const float* W = isx ? p.w_x : p.w_hh;
    const int ldw = isx ? p.ldwx : S;
    const bool wv = !isx || n0 + li < fs;                   // (x tiles: columns at or past fs are the z/c weights - zeros instead)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        wreg[u][e] = wv ? ag_rbf_if(W[(int64_t)((wid * NU + u) * 16 + 4 * g + e) * ldw + n0 + li], RB) : 0.f;
  }
  // h tiles: wp[u][e] = W_p[(wid*NP + u)*16 + 4g + e][n0 + li]
  // (rows at or past fs lie outside W_p: zeros; a lane's 4 k are all inside or all outside since fs % 4 == 0)
  const bool pw_on = !isx && (wid * NP * 16 < fs);
  float wp[NP][4];
  bool pkv[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    pkv[u] = pw_on && (wid * NP + u) * 16 + 4 * g < fs;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      wp[u][e] = pkv[u] ? ag_rbf_if(p.w_p[(int64_t)((wid * NP + u) * 16 + 4 * g + e) * S + n0 + li], RB) : 0.f;
  }

  unsigned* flags_h = p.ctl.hdr + PS_FLAG_OFF + bt * NT;
  unsigned* flags_x = flags_h + NHT;
  unsigned* my_flag = flags_h + ct;
  // epilogue role: thread <-> (clip row, column of the tile)
  const int erow = tid >> 4, ecol = tid & 15;
  const int em = m0 + erow;
  const bool epi = em < B && (!isx || n0 + ecol < fs);      // (x tiles: columns at or past fs do not exist)
  // A operand rows of this lane for the two 16-clip halves (clamped: rows past the batch feed only their own, unwritten outputs)
  const int ar0 = min(m0 + li, B - 1), ar1 = min(m0 + 16 + li, B - 1);
  float carry = 0.f, dcn = 0.f, direct = 0.f;
  bool alive = true;

  for (int t = T - 1; t >= 0; --t) {
    const unsigned seq = (unsigned)(T - t);
    if (isx) {
      if (epi) {
        const float dx = (p.dx_ext ? p.dx_ext[(int64_t)em * p.lddx + (int64_t)t * fs + n0 + ecol] : 0.f) + carry;
        const float xv = p.x[(int64_t)em * p.ldx + (int64_t)t * fs + n0 + ecol];
        float gx = dx * (1.f - xv * xv);
        if (s_dead) gx = __builtin_nanf("");
        __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(p.dxt + (int64_t)t * BX, 0, (int)(BX * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(gx), orr, (unsigned)(((int64_t)em * fs + n0 + ecol) * 4), 0, 16);
      }
    } else {
      float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cp = 0.f, cn = 0.f, ext = 0.f;
      if (epi) {
        const float* gr = p.ga + (int64_t)t * BG + (int64_t)em * K4 + n0 + ecol;
        ig = gr[0]; fg = gr[S]; gg = gr[2 * S];            // LSTM: i, f, g (, o)   GRU: r, z, n
        cp = p.c_all[(int64_t)t * BH + (int64_t)em * S + n0 + ecol];              // c_{t-1}  /  h_{t-1}
        if (CELL == 1) {
          og = p.gh[(int64_t)t * BG + (int64_t)em * K4 + 2 * S + n0 + ecol];      // W_hn h_{t-1} + b_hn
        } else {
          og = gr[3 * S];
          cn = p.c_all[(int64_t)(t + 1) * BH + (int64_t)em * S + n0 + ecol];
        }
        ext = p.dh_ext ? p.dh_ext[(int64_t)t * BH + (int64_t)em * S + n0 + ecol] : 0.f;
      }
      if (wid == 0 && alive) {
        alive = ps_wait_flags<true>(p.ctl, flags_x, NXT, seq, lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
      // gx_t [32 clips, fs] x W_p panel
      f32x4 pa[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
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
              pa[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag_rbf_if(__uint_as_float(a[r][u][e]), RB), wp[u][e], pa[r], 0, 0, 0);
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
        __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(p.dgs + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
        const unsigned o = (unsigned)(((int64_t)em * K4 + n0 + ecol) * 4);
        if (CELL == 1) {
          // torch.nn.GRUCell backward: r = ig, z = fg, n = gg, hn = og, h_{t-1} = cp
          float dn = dhv * (1.f - fg) * (1.f - gg * gg);
          float dz = dhv * (cp - gg) * fg * (1.f - fg);
          float dr = dn * og * ig * (1.f - ig);
          float dnr = dn * ig;
          direct = dhv * fg;                                  // the direct path dh * z, added to frame t-1's dh
          if (s_dead) { dn = dz = dr = dnr = direct = __builtin_nanf(""); }
          __amdgpu_buffer_rsrc_t hrr = __builtin_amdgcn_make_buffer_rsrc(p.dgh + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dr), orr, o, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dz), orr, o + (unsigned)(S * 4), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dn), orr, o + (unsigned)(2 * S * 4), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dr), hrr, o, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dz), hrr, o + (unsigned)(S * 4), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dnr), hrr, o + (unsigned)(2 * S * 4), 0, 16);
        } else {
          const float tc = tanhf(cn);
          const float dc = dcn + dhv * og * (1.f - tc * tc);
          float d0 = dc * gg * ig * (1.f - ig);
          float d1 = dc * cp * fg * (1.f - fg);
          float d2 = dc * ig * (1.f - gg * gg);
          float d3 = dhv * tc * og * (1.f - og);
          dcn = dc * fg;
          if (s_dead) { d0 = d1 = d2 = d3 = dcn = __builtin_nanf(""); }   // a wait timed out: poison instead of garbage
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d0), orr, o, 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d1), orr, o + (unsigned)(S * 4), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d2), orr, o + (unsigned)(2 * S * 4), 0, 16);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d3), orr, o + (unsigned)(3 * S * 4), 0, 16);
        }
      }
    }
    if (t == 0 && !isx) break;                                // dgates_0 has no reader inside the launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // EVERY storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
      __hip_atomic_store(my_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) break;
    // ---- the recurrent term of frame t-1: dgates_t [32 clips, 4S] x panel
    if (wid == 0 && alive) {
      alive = ps_wait_flags(p.ctl, flags_h, NHT, seq, lane);
      if (!alive) s_dead = 1;
    }
    __syncthreads();
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    {
      __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc((isx ? p.dgs : p.dgh) + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
      const unsigned o0 = (unsigned)(((int64_t)ar0 * K4 + wid * NU * 16 + 4 * g) * 4);
      const unsigned o1 = (unsigned)(((int64_t)ar1 * K4 + wid * NU * 16 + 4 * g) * 4);
      constexpr int UB = NU < 4 ? NU : 4;
#pragma unroll
      for (int ub = 0; ub < NU; ub += UB) {
        u32x4 a[2][UB];
#pragma unroll
        for (int i = 0; i < UB; ++i) {
          a[0][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o0 + (unsigned)((ub + i) * 64), 0, 16);
          a[1][i] = __builtin_amdgcn_raw_buffer_load_b128(gr, o1 + (unsigned)((ub + i) * 64), 0, 16);
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
    carry = direct;                                           // (GRU h tiles: dh_t * z_t; otherwise 0)
#pragma unroll
    for (int w = 0; w < 8; ++w) carry += red[w * 512 + tid];
    __syncthreads();                                          // red is written again in the next frame
  }
}

// workgroups of the backward: per clip tile S/16 h tiles and ceil(fs/16) x tiles
static int front_bwd_grid(int B, int S, int fs) { return ag_cdiv(B, 32) * (S / 16 + ag_cdiv(fs, 16)); }

static bool front_bwd_shape_ok(int B, int S, int fs, int n_cu) {
  if (!front_fs_ok(S, fs)) return false;
  if (B < 1) return false;
  if (n_cu > 256) n_cu = 256;
  const int64_t grid = front_bwd_grid(B, S, fs);
  return grid <= n_cu && grid <= (PS_HDR_BYTES / 4 - PS_FLAG_OFF);
}

extern "C" int ag_gfront_bwd_persist_ok(int B, int S, int fs, int n_cu) { return front_bwd_shape_ok(B, S, fs, n_cu) ? 1 : 0; }

// The frame loop of the front's backward through time in ONE launch, LSTM and GRU cell.  Tensor contracts:
// ag_front_bwd_args (include/audiogan_hip.h).  Shapes: ag_gfront_bwd_persist_ok.
extern "C" int ag_gfront_bwd(const ag_front_bwd_args* a, void* stream) {
  static const char* const who = "ag_gfront_bwd";
  if (int rc = front_struct_ok(who, a, "ag_front_bwd_args")) return rc;
  AG_REQUIRE(a->cell == 0 || a->cell == 1, "%s: cell must be 0 (LSTM) or 1 (GRU)", who);
  const bool gru = a->cell == 1;
  const FrontField fields[] = {
      {"ga", a->ga, true}, {"state", a->state, true}, {"gh", a->gh, gru}, {"x", a->x, true},
      {"dh_ext", a->dh_ext, a->dh_ext != nullptr}, {"dx_ext", a->dx_ext, a->dx_ext != nullptr},      // (optional)
      {"w_hh", a->w_hh, true}, {"w_x", a->w_x, true}, {"w_p", a->w_p, true}, {"dgs", a->dgs, true}, {"dgh", a->dgh, gru},
      {"dxt", a->dxt, true}, {"ws", a->ws, true}};
  if (int rc = front_fields_ok(who, fields)) return rc;
  const int T = a->T, B = a->B, S = a->S, fs = a->fs;
  AG_REQUIRE(T > 0, "%s: T must be positive", who);
  AG_REQUIRE(a->ldx >= (int64_t)T * fs && (!a->dx_ext || a->lddx >= (int64_t)T * fs), "%s: row pitch smaller than a row", who);
  if (!front_bwd_shape_ok(B, S, fs, a->n_cu)) {
    ag_set_error("%s: shape B=%d S=%d fs=%d is not supported on %d CUs", who, B, S, fs, a->n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  AG_REQUIRE(a->ldwx >= fs, "%s: bad row pitch", who);
  AG_REQUIRE((int64_t)B * 4 * S * 4 < ((int64_t)1 << 31), "%s: frame slab too large", who);
  AG_REQUIRE((((uintptr_t)a->dgs | (uintptr_t)a->dxt) & 15) == 0, "%s: outputs must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  FrontBwdP p;
  if (int rc = persist_begin(who, a->ws, a->ws_bytes, PS_STICKY_BYTES + PS_HDR_BYTES, st, &p.ctl)) return rc;
  p.ga = a->ga; p.c_all = a->state; p.x = a->x; p.ldx = a->ldx; p.dh_ext = a->dh_ext; p.dx_ext = a->dx_ext; p.lddx = a->lddx;
  p.w_hh = a->w_hh; p.w_x = a->w_x; p.w_p = a->w_p; p.dgs = a->dgs; p.dxt = a->dxt;
  p.gh = a->gh; p.dgh = gru ? a->dgh : a->dgs;      // (LSTM: the field is not read)
  p.T = T; p.B = B; p.ldwx = a->ldwx; p.fs = fs;
  const bool rb = ag_precision() == AG_PREC_BF16;
  const int grid = front_bwd_grid(B, S, fs);
  void (*kern)(const FrontBwdP);
  if (!gru)
    kern = S == 1024 ? (rb ? gfront_persist_bwd_kernel<1024, 256, true, 0> : gfront_persist_bwd_kernel<1024, 256, false, 0>)
                     : (rb ? gfront_persist_bwd_kernel<128, 64, true, 0> : gfront_persist_bwd_kernel<128, 64, false, 0>);
  else
    kern = S == 1024 ? (rb ? gfront_persist_bwd_kernel<1024, 256, true, 1> : gfront_persist_bwd_kernel<1024, 256, false, 1>)
                     : (rb ? gfront_persist_bwd_kernel<128, 64, true, 1> : gfront_persist_bwd_kernel<128, 64, false, 1>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, p);
  AG_CHECK_LAUNCH(who);
  return AG_OK;
}

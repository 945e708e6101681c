// lstm_persist.hip -- a whole NN.LSTM layer pass (audiogan.py:498-503, :543; Embedder :315) as ONE persistent launch
// with the recurrent weights resident in LDS.
//
// The per-step launches of lstm_step.hip re-stream W_hh from the fabric on every one of the T steps (L2 is not kept
// across launches): 8.4 MB per step for the critic's biLSTM, more than the step's own operands.  Here every workgroup
// keeps ITS slice of W_hh in LDS for the whole sequence and only the hidden state crosses workgroups:
//
//   workgroup  = (direction d, batch tile of 32*RT clips, unit tile of 8 hidden units)      1 per CU, all co-resident
//   LDS        = W_hh rows of its 4 gates x 8 units  [32 gate columns][H]  (128 B * H)  + the K-slice reduction buffer
//   per step   : wait until the 64 unit tiles of its (d, batch tile) GROUP have published h_{k-1}  (one flag each)
//                -> A = h_{k-1} rows of the batch tile, straight from L2 into registers (sc1 loads: L1 is never
//                   refreshed by other CUs' stores, MI355X_MICROARCH.md "inter-workgroup visibility")
//                -> gates = pre_k + A * W_slice^T on v_mfma_f32_32x32x2_f32 (K split over the waves, LDS reduction)
//                -> cell non-linearity; c stays in a register for the whole sequence
//                -> publish h_k: write-through (sc1) stores, every wave drains, barrier, one flag store.
//
// Forward exchange buffer layout [parity][group][unit tile q][row][8 units]: a producer writes 1-2 KB contiguous, a
// consumer lane reads one float4 = 4 consecutive k of its row (k = 8q + 4*(lane>>5) + e, the k-slot order of the MFMA),
// 64 lanes covering 1 KB contiguous.  Two parities suffice: h_{k+1} is written only after every group member has
// finished step k, i.e. after it has read h_{k-1}.
//
// Synchronisation is placement independent (agent-scope flags + write-through payload, Guideline 16 R1); every spin is
// bounded by wall clock (s_memrealtime) and reports through a status word instead of hanging.  ONE such launch may be
// in flight per device (all its workgroups must be co-resident).
//
// The generator fronts' persistent launches (front_persist.hip, front_stack.hip) share this file's workspace layout,
// control block and flag wait: persist_common.h.
#include "persist_common.h"

// test hook (ag_persist_debug): a shorter timeout and one workgroup that never publishes its flags, to exercise the
// give-up path on purpose.  ONE-SHOT and per thread: it arms the NEXT persistent launch issued by the calling thread and
// is consumed by it (like ag_bind_workspace), so a test that dies between arming and launching cannot leave a 2-ms
// timeout behind for the rest of the process.
static thread_local unsigned long long g_ps_timeout = PS_TIMEOUT_TICKS;
static thread_local int g_ps_mute = -1;

extern "C" int ag_persist_debug(int64_t timeout_ticks, int mute_block) {
  g_ps_timeout = timeout_ticks > 0 ? (unsigned long long)timeout_ticks : PS_TIMEOUT_TICKS;
  g_ps_mute = mute_block;
  return AG_OK;
}

// (persist_common.h: ps_ctl, for the launchers of every translation unit - the state above stays private to this one)
void ps_debug_take(unsigned long long* timeout, int* mute) {
  *timeout = g_ps_timeout;
  *mute = g_ps_mute;
  g_ps_timeout = PS_TIMEOUT_TICKS;
  g_ps_mute = -1;
}

struct PersistDir {
  float* pre;          // [T,B,4H] in: x-projection (+ biases); out: activated gates
  const float* whh;    // [4H,H]
  float* c_all;        // [T+1,B,H]  (c_all[0] is written 0 by the launch)
  const float* cb;     // optional [B,4H] time-invariant part of the pre-activations
};

struct PersistFwdP {
  PersistDir d[2];
  float* y;            // [T,B,ndir*H]  (y16 != 0: the same tensor as bfloat16 - the pointer then addresses 2-byte elements)
  int y16;
  const int64_t* valid;
  float* xbuf;         // exchange buffer
  PersistCtl ctl;
  int T, B, H, ndir;
  int nbt;             // batch tiles
  int ntile;           // H / 8
  int rb;              // AG_PREC_BF16: both operands of the recurrent product rounded to bf16
};

// PM (precision mode of the recurrent product): 0 = fp32 operands on the fp32 MFMA; 1 = AG_PREC_BF16 with operands
// rounded in registers in front of the fp32 MFMA (shapes whose K slices are not multiples of 16); 2 = AG_PREC_BF16 on
// v_mfma_f32_32x32x16_bf16: W_hh slice in LDS as bf16 (8 k per 16-byte piece), h rows packed on load.
template <int RT, int PM>      // 32-clip row tiles per workgroup
__global__ __launch_bounds__(512) void lstm_persist_fwd_kernel(const PersistFwdP p) {
  constexpr bool RB = PM == 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NKS = 8 / RT;                 // K slices (waves per row tile)
  constexpr int ROWS = 32 * RT;
  const int H = p.H, B = p.B, T = p.T, ntile = p.ntile;
  float* wl = smem;                           // [ntile][2][32][4]
  float* red = smem + (size_t)32 * H;         // [8 waves][1024]
  __shared__ int s_dead;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  if (tid == 0) s_dead = 0;
  const int ngroups = p.ndir * p.nbt;
  const int grp = blockIdx.x % ngroups, ut = blockIdx.x / ngroups;    // a group's blocks share blockIdx % ngroups
  const int dir = grp / p.nbt, bt = grp % p.nbt;
  const PersistDir& D = p.d[dir];
  const int u0 = ut * 8, row0 = bt * ROWS;

  // ---- W_hh slice -> LDS, once: column j = gate (j>>3), unit u0 + (j&7);  element (q, hslot, j, e) = W[row(j)][8q+4hslot+e]
  if (PM == 2) {      // bf16 image: piece (q, j) = W[row(j)][8q .. 8q+7] as 8 bf16
    const int k8n = H >> 3;
    for (int idx = tid; idx < 32 * k8n; idx += 512) {
      const int j = idx / k8n, q = idx - j * k8n;
      const float* src = D.whh + (int64_t)((j >> 3) * H + u0 + (j & 7)) * H + 8 * q;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
      ps_u32x4 r = {ag_pack_bf16(a[0], a[1]), ag_pack_bf16(a[2], a[3]), ag_pack_bf16(b[0], b[1]), ag_pack_bf16(b[2], b[3])};
      *reinterpret_cast<ps_u32x4*>(wl + ((size_t)q * 32 + j) * 4) = r;
    }
  } else {
    const int k4n = H >> 2;
    for (int idx = tid; idx < 32 * k4n; idx += 512) {
      const int j = idx / k4n, k4 = idx - j * k4n;
      const f32x4 v = ag_rbf4_if(*reinterpret_cast<const f32x4*>(D.whh + (int64_t)((j >> 3) * H + u0 + (j & 7)) * H + 4 * k4), RB);
      *reinterpret_cast<f32x4*>(wl + ((size_t)((k4 >> 1) * 2 + (k4 & 1)) * 32 + j) * 4) = v;
    }
  }
  __syncthreads();

  unsigned* flags = p.ctl.hdr + PS_FLAG_OFF + grp * ntile;
  const int64_t xg = (int64_t)ntile * ROWS * 8;                       // floats per (parity, group)
  __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(p.xbuf, 0, (int)(2 * (int64_t)ngroups * xg * 4), 0x00020000);

  // epilogue role: thread <-> (clip row, unit) for the whole sequence; c and h live in registers
  const int erow = tid >> 3, euu = tid & 7;
  const bool ethread = tid < ROWS * 8;
  const int em = row0 + erow, eu = u0 + euu;
  const bool epi = ethread && em < B;
  const int64_t vlen = (epi && p.valid) ? p.valid[em] : ((int64_t)1 << 60);
  float creg = 0.f, hreg = 0.f;
  // accumulator element of (row i, column j) in a 32x32 tile: lane = j + 32*((i>>2)&1), e = (i&3) + 4*(i>>3)
  const int ei = erow & 31, ert = erow >> 5;
  const int ee = (ei & 3) + 4 * (ei >> 3), ehq = (ei >> 2) & 1;

  // MFMA role
  const int rt = RT == 2 ? (wid & 1) : 0, ks = RT == 2 ? (wid >> 1) : wid;
  const int QW = ntile / NKS, q0w = ks * QW;
  bool alive = true;

  // The epilogue's operands.  The pre-activations of step k + 1 are requested at the END of step k, after the flag and BEFORE the
  // trailing gate / cell / output stores, and nothing is written at the top of the loop: the ISA of the previous form began every
  // step with s_waitcnt vmcnt(3) ... vmcnt(0) in front of the re-initialisation of these registers, i.e. with a wait for the
  // previous step's trailing stores to COMPLETE - the very stores that were moved behind the flag so that nobody would wait for
  // them (profiles/r04_lstm_fwd_isa_skeleton.txt).  The time-invariant part is read once.
  bool sv_pad = false;
  float sv_ig = 0.f, sv_fg = 0.f, sv_gg = 0.f, sv_og = 0.f, sv_y = 0.f;
  float pre4[4] = {0.f, 0.f, 0.f, 0.f}, cb4[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_pre = [&](int kk) {
    if (epi) {
      const int tt = dir == 0 ? kk : T - 1 - kk;
      const float* pr = D.pre + ((int64_t)tt * B + em) * 4 * H + eu;
      pre4[0] = pr[0]; pre4[1] = pr[H]; pre4[2] = pr[2 * H]; pre4[3] = pr[3 * H];
    }
  };
  if (epi && D.cb) {
    const float* cb = D.cb + (int64_t)em * 4 * H + eu;
    cb4[0] = cb[0]; cb4[1] = cb[H]; cb4[2] = cb[2 * H]; cb4[3] = cb[3 * H];
  }
  load_pre(0);
  for (int k = 0; k < T; ++k) {
    const int t = dir == 0 ? k : T - 1 - k;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (k > 0) {
      // (polling from wave 7, which with 32-clip tiles has no epilogue loads or stores in flight for the poll's in-order
      // s_waitcnt vmcnt(0) to retire behind, measured the same: 7.9 / 5.6 vs 8.1 / 5.5 us per step)
      alive = ps_wait_group(p.ctl, flags, ntile, (unsigned)k, wid, lane, alive, &s_dead);
      const int par = (k - 1) & 1;
      // byte offset of (q, row, 4*hh) in the exchange buffer
      const unsigned abase = (unsigned)((((int64_t)(par * ngroups + grp) * xg) + (int64_t)(rt * 32 + l31) * 8 + 4 * hh) * 4);
      const float* wrow = wl + ((size_t)hh * 32 + l31) * 4;
      if (PM == 2) {
        // one MFMA per 16 k: lane half hh takes units 8*(2Q+hh) .. +7 of its row = one 32-byte row of tile 2Q+hh
        const unsigned ab2 = (unsigned)((((int64_t)(par * ngroups + grp) * xg) + (int64_t)(rt * 32 + l31) * 8) * 4);
        const float* w2 = wl + (size_t)l31 * 4;
        for (int qb = 0; qb < QW; qb += 16) {
          u32x4 a0[8], a1[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int q = q0w + min(qb + 2 * i, QW - 2) + hh;
            a0[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, ab2 + (unsigned)(q * ROWS * 32), 0, 16);
            a1[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, ab2 + (unsigned)(q * ROWS * 32) + 16u, 0, 16);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            if (qb + 2 * i < QW) {
              const int q = q0w + qb + 2 * i + hh;
              const ps_bf16x8 b = *reinterpret_cast<const ps_bf16x8*>(w2 + (size_t)q * 128);
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ps_pack8(a0[i], a1[i]), b, acc, 0, 0, 0);
            }
          }
        }
      } else
      for (int qb = 0; qb < QW; qb += 8) {
        u32x4 a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int q = q0w + min(qb + i, QW - 1);
          a[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, abase + (unsigned)(q * ROWS * 32), 0, 16 /* sc1 */);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (qb + i < QW) {
            const int q = q0w + qb + i;
            const f32x4 b = *reinterpret_cast<const f32x4*>(wrow + (size_t)q * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(RB ? ag_rbf(__uint_as_float(a[i][e])) : __uint_as_float(a[i][e]), b[e], acc, 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wid * 1024 + e * 64 + lane] = acc[e];
    __syncthreads();
    if (epi) {
      float g4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float s = pre4[g] + cb4[g];
        if (k > 0) {
#pragma unroll
          for (int s_ = 0; s_ < NKS; ++s_) {
            const int w = RT == 2 ? (ert + 2 * s_) : s_;
            s += red[w * 1024 + ee * 64 + 32 * ehq + 8 * g + euu];
          }
        }
        g4[g] = s;
      }
      const bool padded = t >= vlen;
      float yv = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f;
      if (!padded) {
        ig = ag_sigmoid(g4[0]); fg = ag_sigmoid(g4[1]); gg = tanhf(g4[2]); og = ag_sigmoid(g4[3]);
        creg = fg * creg + ig * gg;
        hreg = og * tanhf(creg);
        yv = hreg;
      }
      if (s_dead) { creg = hreg = yv = ig = __builtin_nanf(""); }     // a wait timed out: poison instead of garbage
      // publish h_k FIRST (write-through); the stores nobody waits for (gates, cell, output) go out after the flag
      if (k + 1 < T) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hreg), xr,
            (unsigned)(((int64_t)((k & 1) * ngroups + grp) * xg + ((int64_t)ut * ROWS + erow) * 8 + euu) * 4), 0, 16 /* sc1 */);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // EVERY storing wave drains its write-through stores
      }
      sv_pad = padded; sv_ig = ig; sv_fg = fg; sv_gg = gg; sv_og = og; sv_y = yv;
    } else if (ethread && k + 1 < T) {
      // rows past the batch: keep the exchange buffer defined (the consumers' MFMA rows that read it are never stored)
      __builtin_amdgcn_raw_buffer_store_b32(0u, xr,
          (unsigned)(((int64_t)((k & 1) * ngroups + grp) * xg + ((int64_t)ut * ROWS + erow) * 8 + euu) * 4), 0, 16);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (k + 1 < T) {
      __syncthreads();
      if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
        __hip_atomic_store(flags + ut, (unsigned)(k + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      load_pre(k + 1);
    }
    if (epi) {
      if (!sv_pad) {
        float* pr = D.pre + ((int64_t)t * B + em) * 4 * H + eu;
        pr[0] = sv_ig; pr[H] = sv_fg; pr[2 * H] = sv_gg; pr[3 * H] = sv_og;
      }
      if (k == 0) D.c_all[(int64_t)em * H + eu] = 0.f;         // c_0 = 0: written here, so the caller need not fill it
      D.c_all[((int64_t)(k + 1) * B + em) * H + eu] = creg;
      const int64_t yi = ((int64_t)t * B + em) * p.ndir * H + (int64_t)dir * H + eu;
      if (p.y16) reinterpret_cast<unsigned short*>(p.y)[yi] = (unsigned short)(ag_pack_bf16(sv_y, sv_y) & 0xFFFFu);
      else p.y[yi] = sv_y;
    }
  }
}

static bool persist_shape_ok(int B, int H, int ndir, int n_cu, int* rt_out, int* nbt_out) {
  if (H % 64 != 0 || H < 64 || H > 768 || B < 1) return false;
  if (n_cu > 256) n_cu = 256;
  const int ntile = H / 8;
  // one workgroup per CU, all co-resident: take 64-clip tiles when 32-clip tiles would not fit the chip
  for (int rt = 1; rt <= 2; ++rt) {
    const int nbt = ag_cdiv(B, 32 * rt);
    if ((int64_t)ndir * nbt * ntile <= n_cu && ndir * nbt * ntile <= (PS_HDR_BYTES / 4 - PS_FLAG_OFF)) {
      *rt_out = rt;
      *nbt_out = nbt;
      return true;
    }
  }
  return false;
}

extern "C" int ag_lstm_persist_ok(int B, int H, int ndir, int n_cu) {
  int rt, nbt;
  return persist_shape_ok(B, H, ndir, n_cu, &rt, &nbt) ? 1 : 0;
}

extern "C" int64_t ag_lstm_persist_ws_bytes(int B, int H, int ndir) {
  // header + 2 parities of the padded hidden state, both directions (64-clip padding covers both tilings)
  return PS_STICKY_BYTES + PS_HDR_BYTES + (int64_t)2 * ndir * ag_roundup(B, 64) * H * 4;
}

// Whole (bi)directional layer forward in ONE launch.  Same tensors as ag_lstm_seq_fwd (lstm_step.hip) minus the
// hidden-state scratch; `ws` = ag_lstm_persist_ws_bytes() bytes of device memory, 16-byte aligned, used by no other
// launch in flight.  `n_cu`: compute units of the device (the grid must be co-resident).
extern "C" int ag_lstm_seq_fwd_persist(float* const* pre, const float* const* whh, float* const* c_all, void* y, int y_bf16,
                                       const int64_t* valid_i64, const float* const* static_pre, void* ws,
                                       int64_t ws_bytes, int T, int B, int H, int ndir, int n_cu, void* stream) {
  AG_REQUIRE(pre && whh && c_all && y && ws, "ag_lstm_seq_fwd_persist: null tensor");
  AG_REQUIRE(ndir == 1 || ndir == 2, "ag_lstm_seq_fwd_persist: ndir must be 1 or 2");
  AG_REQUIRE(T > 0, "ag_lstm_seq_fwd_persist: T must be positive");
  int rt = 0, nbt = 0;
  if (!persist_shape_ok(B, H, ndir, n_cu, &rt, &nbt)) {
    ag_set_error("ag_lstm_seq_fwd_persist: shape B=%d H=%d ndir=%d does not fit %d CUs", B, H, ndir, n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  for (int d = 0; d < ndir; ++d) AG_REQUIRE(((uintptr_t)whh[d] & 15) == 0, "ag_lstm_seq_fwd_persist: W_hh must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  PersistFwdP p;
  if (int rc = persist_begin("ag_lstm_seq_fwd_persist", ws, ws_bytes, ag_lstm_persist_ws_bytes(B, H, ndir), st, &p.ctl)) return rc;
  for (int d = 0; d < 2; ++d) {
    const int s = d < ndir ? d : 0;
    p.d[d].pre = pre[s]; p.d[d].whh = whh[s]; p.d[d].c_all = c_all[s];
    p.d[d].cb = static_pre ? static_pre[s] : nullptr;
  }
  p.y = (float*)y; p.y16 = y_bf16 ? 1 : 0; p.valid = valid_i64;
  p.xbuf = (float*)((char*)ws + PS_STICKY_BYTES + PS_HDR_BYTES);
  p.T = T; p.B = B; p.H = H; p.ndir = ndir; p.nbt = nbt; p.ntile = H / 8;
  p.rb = ag_precision() == AG_PREC_BF16;
  const size_t lds = ((size_t)32 * H + 8 * 1024) * sizeof(float);
  const int grid = ndir * nbt * p.ntile;
  // bf16 mode: the bf16 MFMA needs 16-k steps inside a wave's K slice (H/8 unit tiles over 8/rt waves, 2 tiles a step)
  const int pm = !p.rb ? 0 : ((p.ntile / (8 / rt)) % 2 == 0 ? 2 : 1);
  void (*kern)(const PersistFwdP) =
      rt == 1 ? (pm == 0 ? lstm_persist_fwd_kernel<1, 0> : pm == 1 ? lstm_persist_fwd_kernel<1, 1> : lstm_persist_fwd_kernel<1, 2>)
              : (pm == 0 ? lstm_persist_fwd_kernel<2, 0> : pm == 1 ? lstm_persist_fwd_kernel<2, 1> : lstm_persist_fwd_kernel<2, 2>);
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, p);
  AG_CHECK_LAUNCH("ag_lstm_seq_fwd_persist");
  return AG_OK;
}

// ------------------------------------------------------------------------------------------
// Backward through time as ONE persistent launch.
//
//   dh_k[m,u] = sum_kk dgates_{k+1}[m,kk] * W_hh[kk,u]  (+ pass-through of padded rows),   K = 4H
//   (dgates_k, dc, pass-through) = cell backward of step k
//
// The contraction runs over ALL 4H gate columns, so a workgroup that owns 32 hidden units needs the W_hh slice
// [4H x 32] = 256 KB at H = 512: more than LDS, but not more than the REGISTER FILE (512 KB per CU).  Each of the
// 8 waves keeps its K slice of that panel in VGPRs for the whole sequence (4H/8 k-values x 32 units = 128 registers
// per lane at H = 512) as ready-made MFMA B operands; nothing but dgates is read per step.
//
//   workgroup = (direction, 16-clip tile, 32-unit tile); group = the H/32 unit tiles of one (direction, clip tile)
//   per step  : wait for the group's flags -> A = dgates_{k+1}[16 clips, K slice] (sc1 loads, straight from L2)
//               -> v_mfma_f32_16x16x4_f32 against the resident panel -> LDS sum of the 8 K slices
//               -> cell backward for its (clip, unit) pairs; dc and the pass-through stay in registers
//               -> dgates_k written THROUGH (sc1) into the output tensor itself, which is also the exchange
//                  buffer (one slot per step: no parity), every wave drains, barrier, flag.
// ------------------------------------------------------------------------------------------
struct PersistBwdDir {
  const float* ga;      // [T,B,4H] activated gates
  const float* whh;     // [4H,H]
  const float* c_all;   // [T+1,B,H]
  float* dgates;        // [T,B,4H] out (and exchange)
  float* dgsum;         // optional [B,4H] out: sum over time of dgates (what the biases and a time-invariant input see)
  unsigned short* dg16; // optional [T,B,4H] out (row pitch dg16_ld): dgates as bfloat16, the operand of the gradient products
};

struct PersistBwdP {
  PersistBwdDir d[2];
  const float* dy;      // [T,B,ndir*H]  (dy16 != 0: stored as bfloat16, the pointer addresses 2-byte elements)
  int dy16;
  int dg16_ld;          // row pitch of dg16 in elements (>= 4H: both directions may share one [T,B,ndir*4H] tensor)
  const int64_t* valid;
  PersistCtl ctl;
  int T, B, H, ndir;
  int nbt;              // 16-clip tiles
  int ntile;            // H / 32
  int rb;               // AG_PREC_BF16: both operands of the recurrent product rounded to bf16
};

// PM: 0 = fp32; 2 = AG_PREC_BF16 on v_mfma_f32_16x16x32_bf16 (the W_hh panel in registers as bf16: half the VGPRs)
template <int NU, int PM>       // 16-k units per wave: 4H = 8 waves * NU * 16
__global__ __launch_bounds__(512) void lstm_persist_bwd_kernel(const PersistBwdP p) {
  constexpr bool RB = false;
  __shared__ float red[8 * 512];
  __shared__ int s_dead;
  const int H = p.H, B = p.B, T = p.T, ntile = p.ntile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  if (tid == 0) s_dead = 0;
  __syncthreads();
  const int ngroups = p.ndir * p.nbt;
  const int grp = blockIdx.x % ngroups, ut = blockIdx.x / ngroups;
  const int dir = grp / p.nbt, bt = grp % p.nbt;
  const PersistBwdDir& D = p.d[dir];
  const int n0 = ut * 32, m0 = bt * 16;
  const int64_t BG = (int64_t)B * 4 * H, BH = (int64_t)B * H;

  // ---- resident weight panel: wreg[u][e][c] = W_hh[(wid*NU + u)*16 + 4g + e][n0 + 16c + li]
  constexpr int NW = PM == 2 ? 1 : NU;        // (the fp32 panel is not allocated in bf16 mode)
  float wreg[NW][4][2];
  if (PM != 2) {
#pragma unroll
    for (int u = 0; u < NW; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          wreg[u][e][c] = ag_rbf_if(D.whh[(int64_t)((wid * NU + u) * 16 + 4 * g + e) * H + n0 + 16 * c + li], RB);
  }
  // bf16 panel: 32-k steps; wbf[U][c] = W_hh[(wid*NU/2 + U)*32 + 8g + 0..7][n0 + 16c + li]
  constexpr int NU2 = PM == 2 ? NU / 2 : 1;
  ps_bf16x8b wbf[NU2][2];
  if (PM == 2) {
#pragma unroll
    for (int U = 0; U < NU2; ++U)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float* src = D.whh + (int64_t)((wid * NU2 + U) * 32 + 8 * g) * H + n0 + 16 * c + li;
        ps_u32x4 r = {ag_pack_bf16(src[0], src[H]), ag_pack_bf16(src[2 * (int64_t)H], src[3 * (int64_t)H]),
                      ag_pack_bf16(src[4 * (int64_t)H], src[5 * (int64_t)H]), ag_pack_bf16(src[6 * (int64_t)H], src[7 * (int64_t)H])};
        wbf[U][c] = __builtin_bit_cast(ps_bf16x8b, r);
      }
  }

  unsigned* flags = p.ctl.hdr + PS_FLAG_OFF + grp * ntile;
  // epilogue role: thread <-> (clip row, unit)
  const int erow = tid >> 5, eun = tid & 31;
  const int em = m0 + erow, eu = n0 + eun;
  const bool epi = em < B;
  const int64_t vlen = (epi && p.valid) ? p.valid[em] : ((int64_t)1 << 60);
  float dcn = 0.f, dpass = 0.f;
  float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sum3 = 0.f;      // time sums of this thread's four dgates (fixed order: k = T-1 .. 0)
  // A operand row of this lane (clamped: rows past the batch only feed their own, unwritten outputs)
  const int arow = min(m0 + li, B - 1);
  const unsigned aoff = (unsigned)(((int64_t)arow * 4 * H + (wid * NU) * 16 + 4 * g) * 4);
  bool alive = true;

  for (int k = T - 1; k >= 0; --k) {
    const int t = dir == 0 ? k : T - 1 - k;
    float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cp = 0.f, cn = 0.f, dyv = 0.f;
    if (epi) {
      const float* gr = D.ga + (int64_t)t * BG + (int64_t)em * 4 * H + eu;
      ig = gr[0]; fg = gr[H]; gg = gr[2 * H]; og = gr[3 * H];
      cp = D.c_all[(int64_t)k * BH + (int64_t)em * H + eu];
      cn = D.c_all[(int64_t)(k + 1) * BH + (int64_t)em * H + eu];
      const int64_t yi = ((int64_t)t * B + em) * p.ndir * H + (int64_t)dir * H + eu;
      dyv = p.dy16 ? __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(p.dy)[yi] << 16) : p.dy[yi];
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (k < T - 1) {
      alive = ps_wait_group(p.ctl, flags, ntile, (unsigned)(T - 1 - k), wid, lane, alive, &s_dead);
      const int tn = dir == 0 ? k + 1 : T - 2 - k;
      __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(D.dgates + (int64_t)tn * BG, 0, (int)(BG * 4), 0x00020000);
      if (PM == 2) {
        // lane (clip li, k slot g) takes k = 32U + 8g .. +7 of its dgates row (32 contiguous bytes)
        const unsigned aoff2 = (unsigned)(((int64_t)arow * 4 * H + (wid * NU2) * 32 + 8 * g) * 4);
        u32x4 a0[NU2], a1[NU2];
#pragma unroll
        for (int U = 0; U < NU2; ++U) {
          a0[U] = __builtin_amdgcn_raw_buffer_load_b128(ar, aoff2 + (unsigned)(U * 128), 0, 16);
          a1[U] = __builtin_amdgcn_raw_buffer_load_b128(ar, aoff2 + (unsigned)(U * 128) + 16u, 0, 16);
        }
#pragma unroll
        for (int U = 0; U < NU2; ++U) {
          const ps_bf16x8b av = __builtin_bit_cast(ps_bf16x8b, ps_pack8(a0[U], a1[U]));
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, wbf[U][c], acc[c], 0, 0, 0);
        }
      }
      constexpr int UB = NU < 8 ? NU : 8;
#pragma unroll
      for (int ub = 0; ub < (PM == 2 ? 0 : NU); ub += UB) {
        u32x4 a[UB];
#pragma unroll
        for (int i = 0; i < UB; ++i) a[i] = __builtin_amdgcn_raw_buffer_load_b128(ar, aoff + (unsigned)((ub + i) * 64), 0, 16);
#pragma unroll
        for (int i = 0; i < UB; ++i) {
          float av[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) av[e] = RB ? ag_rbf(__uint_as_float(a[i][e])) : __uint_as_float(a[i][e]);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wreg[PM == 2 ? 0 : ub + i][e][c], acc[c], 0, 0, 0);
        }
      }
    }
    // C layout of a 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + e
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wid * 512 + (4 * g + e) * 32 + 16 * c + li] = acc[c][e];
    __syncthreads();
    if (epi) {
      float dhf = dpass;
      if (k < T - 1) {
#pragma unroll
        for (int w = 0; w < 8; ++w) dhf += red[w * 512 + tid];
      }
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
      if (t >= vlen) {
        dpass = dhf;          // padded step: gradient passes through h and c unchanged
      } else {
        const float dhv = dhf + dyv;
        const float tc = tanhf(cn);
        const float dc = dcn + dhv * og * (1.f - tc * tc);
        d0 = dc * gg * ig * (1.f - ig);
        d1 = dc * cp * fg * (1.f - fg);
        d2 = dc * ig * (1.f - gg * gg);
        d3 = dhv * tc * og * (1.f - og);
        dcn = dc * fg;
        dpass = 0.f;
      }
      if (s_dead) { d0 = d1 = d2 = d3 = dcn = __builtin_nanf(""); }   // a wait timed out: poison instead of garbage
      sum0 += d0; sum1 += d1; sum2 += d2; sum3 += d3;
      if (D.dg16) {
        unsigned short* q16 = D.dg16 + ((int64_t)t * B + em) * p.dg16_ld + eu;
        q16[0] = (unsigned short)(ag_pack_bf16(d0, d0) & 0xFFFFu); q16[H] = (unsigned short)(ag_pack_bf16(d1, d1) & 0xFFFFu);
        q16[2 * H] = (unsigned short)(ag_pack_bf16(d2, d2) & 0xFFFFu); q16[3 * H] = (unsigned short)(ag_pack_bf16(d3, d3) & 0xFFFFu);
      }
      __amdgpu_buffer_rsrc_t orr = __builtin_amdgcn_make_buffer_rsrc(D.dgates + (int64_t)t * BG, 0, (int)(BG * 4), 0x00020000);
      const unsigned o = (unsigned)(((int64_t)em * 4 * H + eu) * 4);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d0), orr, o, 0, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d1), orr, o + (unsigned)(H * 4), 0, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d2), orr, o + (unsigned)(2 * H * 4), 0, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(d3), orr, o + (unsigned)(3 * H * 4), 0, 16);
    }
    if (k > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // EVERY storing wave drains its write-through stores
      __syncthreads();
      if (tid == 0 && (int)blockIdx.x != p.ctl.mute)
        __hip_atomic_store(flags + ut, (unsigned)(T - k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (epi && D.dgsum) {
    float* q = D.dgsum + (int64_t)em * 4 * H + eu;
    q[0] = sum0; q[H] = sum1; q[2 * H] = sum2; q[3 * H] = sum3;
  }
}

static bool persist_bwd_shape_ok(int B, int H, int ndir, int n_cu) {
  if (!(H == 64 || H == 128 || H == 256 || H == 512) || B < 1) return false;
  if (n_cu > 256) n_cu = 256;
  const int64_t grid = (int64_t)ndir * ag_cdiv(B, 16) * (H / 32);
  return grid <= n_cu && grid <= (PS_HDR_BYTES / 4 - PS_FLAG_OFF);
}

extern "C" int ag_lstm_persist_bwd_ok(int B, int H, int ndir, int n_cu) {
  return persist_bwd_shape_ok(B, H, ndir, n_cu) ? 1 : 0;
}

// Whole layer backward through time in ONE launch; tensors as for ag_lstm_seq_bwd (no scratch state: dc and the
// pass-through term stay in registers).  `ws`: >= 8 KiB (status + flags), zeroed by a memset node in front.
extern "C" int ag_lstm_seq_bwd_persist(const float* const* gates, const float* const* whh, const float* const* c_all,
                                       const void* dy, int dy_bf16, float* const* dgates, float* const* dgsum,
                                       uint16_t* const* dg16, int dg16_ld, const int64_t* valid_i64, void* ws,
                                       int64_t ws_bytes, int T, int B, int H, int ndir, int n_cu, void* stream) {
  AG_REQUIRE(gates && whh && c_all && dy && dgates && ws, "ag_lstm_seq_bwd_persist: null tensor");
  AG_REQUIRE(ndir == 1 || ndir == 2, "ag_lstm_seq_bwd_persist: ndir must be 1 or 2");
  AG_REQUIRE(T > 0, "ag_lstm_seq_bwd_persist: T must be positive");
  if (!persist_bwd_shape_ok(B, H, ndir, n_cu)) {
    ag_set_error("ag_lstm_seq_bwd_persist: shape B=%d H=%d ndir=%d does not fit %d CUs", B, H, ndir, n_cu);
    return AG_ERR_UNSUPPORTED;
  }
  AG_REQUIRE((int64_t)B * 4 * H * 4 < ((int64_t)1 << 31), "ag_lstm_seq_bwd_persist: step slab too large");
  AG_REQUIRE(!dg16 || dg16_ld >= 4 * H, "ag_lstm_seq_bwd_persist: dg16 row pitch smaller than a row");
  hipStream_t st = (hipStream_t)stream;
  PersistBwdP p;
  if (int rc = persist_begin("ag_lstm_seq_bwd_persist", ws, ws_bytes, PS_STICKY_BYTES + PS_HDR_BYTES, st, &p.ctl)) return rc;
  for (int d = 0; d < 2; ++d) {
    const int s = d < ndir ? d : 0;
    p.d[d].ga = gates[s]; p.d[d].whh = whh[s]; p.d[d].c_all = c_all[s]; p.d[d].dgates = dgates[s];
    p.d[d].dgsum = dgsum ? dgsum[s] : nullptr;
    p.d[d].dg16 = dg16 ? dg16[s] : nullptr;
  }
  p.dy = (const float*)dy; p.dy16 = dy_bf16 ? 1 : 0; p.dg16_ld = dg16_ld; p.valid = valid_i64;
  p.T = T; p.B = B; p.H = H; p.ndir = ndir; p.nbt = ag_cdiv(B, 16); p.ntile = H / 32;
  p.rb = ag_precision() == AG_PREC_BF16;
  const int grid = ndir * p.nbt * p.ntile;
  void (*kern)(const PersistBwdP);
  switch (H) {
    case 512: kern = p.rb ? lstm_persist_bwd_kernel<16, 2> : lstm_persist_bwd_kernel<16, 0>; break;
    case 256: kern = p.rb ? lstm_persist_bwd_kernel<8, 2> : lstm_persist_bwd_kernel<8, 0>; break;
    case 128: kern = p.rb ? lstm_persist_bwd_kernel<4, 2> : lstm_persist_bwd_kernel<4, 0>; break;
    default:  kern = p.rb ? lstm_persist_bwd_kernel<2, 2> : lstm_persist_bwd_kernel<2, 0>; break;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, p);
  AG_CHECK_LAUNCH("ag_lstm_seq_bwd_persist");
  return AG_OK;
}

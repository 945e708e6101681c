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
#include "common.h"

#include <type_traits>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Workspace layout: [sticky area PS_STICKY_BYTES][header PS_HDR_BYTES][exchange buffers].
//   sticky word 0 : OR of every timeout since the workspace was allocated; NEVER cleared by a launch (a step issues many
//                   persistent launches on one workspace, the host reads this word once per step / bench run)
//   header word 0 : status of THIS launch ("somebody gave up": the other workgroups stop waiting too)
//   header words PS_FLAG_OFF.. : flags.  The header is zeroed by a memset node in front of every launch.
// A workgroup that gave up poisons everything it writes from then on with NaN, so the failure also reaches the loss and
// the optimiser's check_grad flags instead of leaving plausible garbage.
#define PS_STICKY_BYTES 256
#define PS_FLAG_OFF 16
#define PS_HDR_BYTES 8192
#define PS_TIMEOUT_TICKS 300000000ull   // 3 s of the 100 MHz realtime counter

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

struct PersistCtl {
  unsigned* hdr;              // status + flags of this launch
  unsigned* sticky;           // sticky status word
  unsigned long long timeout; // ticks
  int mute;                   // block that never publishes (-1: none)
};

static PersistCtl ps_ctl(void* ws) {
  PersistCtl c;
  c.sticky = (unsigned*)ws;
  c.hdr = (unsigned*)((char*)ws + PS_STICKY_BYTES);
  c.timeout = g_ps_timeout;
  c.mute = g_ps_mute;
  g_ps_timeout = PS_TIMEOUT_TICKS;      // consumed: the hook arms one launch
  g_ps_mute = -1;
  return c;
}

// The prologue of every persistent host launcher: the workspace check, the memset node that zeroes the header, the control
// block.  The LAST step before a launcher fills its parameters: ps_ctl consumes the ag_persist_debug arming, and a call that
// fails validation must not consume it.
static int persist_begin(const char* who, void* ws, int64_t ws_bytes, int64_t need, hipStream_t st, PersistCtl* ctl) {
  AG_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: workspace too small or misaligned", who);
  if (hipMemsetAsync((char*)ws + PS_STICKY_BYTES, 0, PS_HDR_BYTES, st) != hipSuccess) {
    ag_set_error("%s: memset failed", who);
    return AG_ERR_LAUNCH;
  }
  *ctl = ps_ctl(ws);
  return AG_OK;
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

// LE64: the caller guarantees n <= 64 where n is only known at run time - one predicated load per poll instead of a loop
// with a run-time trip count (which cost the fronts' forward 1.5 us per frame when the number of projection tiles became a
// run-time value)
template <bool LE64 = false>
__device__ __forceinline__ bool ps_wait_flags(const PersistCtl& ctl, const unsigned* flags, int n, unsigned want, int lane) {
  unsigned* hdr = ctl.hdr;
  // ONE wave polls the group's flags (lane i <-> flags i, i + 64, ...), relaxed agent-scope loads
  unsigned long long t0 = 0;
  for (unsigned spins = 0;; ++spins) {
    bool ok = true;
    if (LE64) {
      if (lane < n) ok = __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want;
    } else {
      for (int i = lane; i < n; i += 64)
        ok &= __hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want;
    }
    if (__all(ok)) return true;
    if ((spins & 63) == 63) {
      if (__hip_atomic_load(hdr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;   // somebody gave up
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      if (t0 == 0) t0 = now;
      else if (now - t0 > ctl.timeout) {
        if (lane == 0) {
          __hip_atomic_store(hdr, 0x80000000u | want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_or(ctl.sticky, 0x80000000u | want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

typedef short ps_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned ps_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ ps_bf16x8 ps_pack8(u32x4 lo, u32x4 hi) {      // 8 floats (bit patterns) -> 8 bf16, RNE
  ps_u32x4 r = {ag_pack_bf16(__uint_as_float(lo[0]), __uint_as_float(lo[1])), ag_pack_bf16(__uint_as_float(lo[2]), __uint_as_float(lo[3])),
                ag_pack_bf16(__uint_as_float(hi[0]), __uint_as_float(hi[1])), ag_pack_bf16(__uint_as_float(hi[2]), __uint_as_float(hi[3]))};
  return __builtin_bit_cast(ps_bf16x8, r);
}

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
      if (wid == 0 && alive) {
        alive = ps_wait_flags(p.ctl, flags, ntile, (unsigned)k, lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
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

typedef short ps_bf16x8b __attribute__((ext_vector_type(8)));

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
      if (wid == 0 && alive) {
        alive = ps_wait_flags(p.ctl, flags, ntile, (unsigned)(T - 1 - k), lane);
        if (!alive) s_dead = 1;
      }
      __syncthreads();
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

// Generation mode (GEN = 1, ag_gfront_fwd with gen = 1): sampling, no autograd.  No history is written (gates, hs, cs, gh, xt:
// only x); `gates` holds the pre-activations and is only read.  Per frame the projection workgroups of column tile 0 (ut = 0
// and 1: one per 16-clip subtile) also form the stop logit s = h_t . w_s + b_s beside their MFMA tile and draw the stop,
// stop = u[t,b] < sigmoid(s).  Exit rule: every subtile publishes, before its x flag of frame t,
//   gen_all[sub]  (write-once) = t + 1 at the first frame t by which every clip of the subtile has drawn a stop
//   gen_done[sub] = t + 1: the subtile's decisions of frames <= t are final
// At the top of frame t + 1 every workgroup waits for gen_done >= t - GEN_LAG + 1 of ALL subtiles and leaves the loop iff every
// gen_all is in [1, t - GEN_LAG + 1].  Both are final, write-once facts about frame t - GEN_LAG, so every workgroup takes
// the same decision at the same frame and nobody waits for a flag that is never published.  The lag keeps the wait off the
// critical path: the h part of frame t + 1 may start before phase B of frame t has finished anywhere; the GEN_LAG frames run
// past the last stop are correct frames that the caller discards.
#define PS_GEN_OFF (PS_FLAG_OFF + 512)     // header words of the generation mode (the fronts' flags use at most 320)
#define GEN_LAG 1

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
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wid * 1024 + e * 64 + lane] = acc[e];
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

// the padded width of the x panel (the kernels' FS) for a state size, 0 = no instantiation; the fronts take every frame
// size fs % 8 == 0 with 8 <= fs <= this width
static int front_panel(int S) { return S == 1024 ? 256 : S == 128 ? 64 : 0; }
static bool front_fs_ok(int S, int fs) { return fs >= 8 && fs % 8 == 0 && fs <= front_panel(S); }

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

// A pointer field of ag_front_fwd_args / ag_front_bwd_args and whether the chosen (cell, gen) uses it: a used field must
// be set, and a field that is not used must be NULL (a caller that fills a field the launch ignores has mixed up two forms).
struct FrontField {
  const char* name;
  const void* p;
  bool used;
};

template <int N>
static int front_fields_ok(const char* who, const FrontField (&f)[N]) {
  for (const FrontField& e : f)
    AG_REQUIRE((e.p != nullptr) == e.used, "%s: %s %s", who, e.name, e.used ? "is NULL" : "is not used by this cell / mode and must be NULL");
  return AG_OK;
}

// The frame loop of the Generator front in ONE launch: training forward and generation mode, LSTM and GRU cell.  Tensor
// contracts: ag_front_fwd_args (include/audiogan_hip.h).  Shapes: ag_gfront_persist_ok.
extern "C" int ag_gfront_fwd(const ag_front_fwd_args* a, void* stream) {
  static const char* const who = "ag_gfront_fwd";
  AG_REQUIRE(a && a->struct_bytes == (int64_t)sizeof(*a), "%s: struct_bytes = %lld, but ag_front_fwd_args has %zu bytes in this library",
             who, a ? (long long)a->struct_bytes : -1LL, sizeof(*a));
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
// [nl][nrt][S/8] h flags, then [nrt][NB] x flags, all counting frames.  Hand-offs as everywhere in this file.
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
#define FRONT_MAX_LAYERS 8

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
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wid * 1024 + e * 64 + lane] = acc[e];
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
  AG_REQUIRE(a && a->struct_bytes == (int64_t)sizeof(*a), "%s: struct_bytes = %lld, but ag_front_stack_args has %zu bytes in this library",
             who, a ? (long long)a->struct_bytes : -1LL, sizeof(*a));
  AG_REQUIRE(a->gen == 0 || a->gen == 1, "%s: gen must be 0 (training) or 1 (generation)", who);
  AG_REQUIRE(a->nl >= 1 && a->nl <= FRONT_MAX_LAYERS, "%s: nl = %d, the per-layer tables hold 1 to %d layers", who, a->nl, FRONT_MAX_LAYERS);
  const bool gen = a->gen == 1;
  const int nl = a->nl;
  static const char* const idx[FRONT_MAX_LAYERS] = {"[0]", "[1]", "[2]", "[3]", "[4]", "[5]", "[6]", "[7]"};
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    const bool in = l < nl;
    const struct { const char* name; const void* p; bool used; } f[] = {
        {"gates", a->gates[l], in && (!gen || l == 0)}, {"hs", a->hs[l], in && !gen}, {"cs", a->cs[l], in && !gen},
        {"w_hh", a->w_hh[l], in}, {"w_in", a->w_in[l], in}, {"bias", a->bias[l], in && l > 0}};
    for (const auto& e : f)
      AG_REQUIRE((e.p != nullptr) == e.used, "%s: %s%s %s", who, e.name, idx[l],
                 e.used ? "is NULL" : (in ? "is not used by this layer / mode and must be NULL" : "lies past nl and must be NULL"));
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
  AG_REQUIRE(a && a->struct_bytes == (int64_t)sizeof(*a), "%s: struct_bytes = %lld, but ag_front_bwd_args has %zu bytes in this library",
             who, a ? (long long)a->struct_bytes : -1LL, sizeof(*a));
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

// ------------------------------------------------------------------------------------------
// Backward through time of a STACKED front (2 to 8 LSTMCell layers, L = nl - 1 the top one) as ONE persistent launch: the
// one-layer launch above with a layer coordinate.  Per frame t = T-1 .. 0 (every term of frame T is zero):
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
  AG_REQUIRE(a && a->struct_bytes == (int64_t)sizeof(*a), "%s: struct_bytes = %lld, but ag_front_stack_bwd_args has %zu bytes in this library",
             who, a ? (long long)a->struct_bytes : -1LL, sizeof(*a));
  AG_REQUIRE(a->nl >= 1 && a->nl <= FRONT_MAX_LAYERS, "%s: nl = %d, the per-layer tables hold 1 to %d layers", who, a->nl, FRONT_MAX_LAYERS);
  const int nl = a->nl;
  static const char* const idx[FRONT_MAX_LAYERS] = {"[0]", "[1]", "[2]", "[3]", "[4]", "[5]", "[6]", "[7]"};
  for (int l = 0; l < FRONT_MAX_LAYERS; ++l) {
    const bool in = l < nl;
    const struct { const char* name; const void* p; } f[] = {
        {"ga", a->ga[l]}, {"cs", a->cs[l]}, {"w_hh", a->w_hh[l]}, {"w_in", a->w_in[l]}, {"dgs", a->dgs[l]}};
    for (const auto& e : f)
      AG_REQUIRE((e.p != nullptr) == in, "%s: %s%s %s", who, e.name, idx[l], in ? "is NULL" : "lies past nl and must be NULL");
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

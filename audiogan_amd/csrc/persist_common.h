// persist_common.h -- what every persistent launch uses (lstm_persist.hip: the NN.LSTM layer pass; front_persist.hip: the
// one-layer generator front; front_stack.hip: the stacked front): the workspace layout, the control block and the host
// prologue, the bounded flag wait and the bf16 packing of MFMA operands.
#pragma once
#include "common.h"

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

struct PersistCtl {
  unsigned* hdr;              // status + flags of this launch
  unsigned* sticky;           // sticky status word
  unsigned long long timeout; // ticks
  int mute;                   // block that never publishes (-1: none)
};

// The test hook's state (ag_persist_debug) lives in lstm_persist.hip, ONCE for the library: this hands out the armed
// timeout and muted block of the calling thread and disarms them.
__attribute__((visibility("hidden"))) void ps_debug_take(unsigned long long* timeout, int* mute);

static inline PersistCtl ps_ctl(void* ws) {
  PersistCtl c;
  c.sticky = (unsigned*)ws;
  c.hdr = (unsigned*)((char*)ws + PS_STICKY_BYTES);
  ps_debug_take(&c.timeout, &c.mute);   // consumed: the hook arms one launch
  return c;
}

// The prologue of every persistent host launcher: the workspace check, the memset node that zeroes the header, the control
// block.  The LAST step before a launcher fills its parameters: ps_ctl consumes the ag_persist_debug arming, and a call that
// fails validation must not consume it.
static inline int persist_begin(const char* who, void* ws, int64_t ws_bytes, int64_t need, hipStream_t st, PersistCtl* ctl) {
  AG_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: workspace too small or misaligned", who);
  if (hipMemsetAsync((char*)ws + PS_STICKY_BYTES, 0, PS_HDR_BYTES, st) != hipSuccess) {
    ag_set_error("%s: memset failed", who);
    return AG_ERR_LAUNCH;
  }
  *ctl = ps_ctl(ws);
  return AG_OK;
}

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

// The wait in front of a hand-off, for the whole workgroup: wave 0 polls while the workgroup is alive, a wait that gave up
// marks the workgroup dead (the returned `alive` of the polling wave, *s_dead for everybody: the poison rule), then the
// barrier behind which the payload may be read.  `alive` goes in and out by value: through a reference the layer kernels'
// instructions came out in another order.  The layer kernels (lstm_persist.hip) call it at every wait; the fronts spell the
// same four lines out at every wait, because at most of their sites the call changed the kernel's instructions
// (profiles/front_parts_isa.txt) and a form used at some sites only is worse than either.
__device__ __forceinline__ bool ps_wait_group(const PersistCtl& ctl, const unsigned* flags, int n, unsigned want, int wid, int lane,
                                              bool alive, int* s_dead) {
  if (wid == 0 && alive) {
    alive = ps_wait_flags(ctl, flags, n, want, lane);
    if (!alive) *s_dead = 1;
  }
  __syncthreads();
  return alive;
}

typedef short ps_bf16x8 __attribute__((ext_vector_type(8)));
typedef short ps_bf16x8b __attribute__((ext_vector_type(8)));
typedef unsigned ps_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ ps_bf16x8 ps_pack8(u32x4 lo, u32x4 hi) {      // 8 floats (bit patterns) -> 8 bf16, RNE
  ps_u32x4 r = {ag_pack_bf16(__uint_as_float(lo[0]), __uint_as_float(lo[1])), ag_pack_bf16(__uint_as_float(lo[2]), __uint_as_float(lo[3])),
                ag_pack_bf16(__uint_as_float(hi[0]), __uint_as_float(hi[1])), ag_pack_bf16(__uint_as_float(hi[2]), __uint_as_float(hi[3]))};
  return __builtin_bit_cast(ps_bf16x8, r);
}

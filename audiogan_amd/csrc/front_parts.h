// front_parts.h -- what the two generator fronts' persistent launches share (front_persist.hip: one layer, LSTM / GRU,
// bf16 MFMAs, generation mode; front_stack.hip: 2 to 8 LSTMCell layers): the host launchers' checks, the generation mode's
// constants and what of the frame loops could be shared without changing either kernel's instructions.  Rule for anything
// added here: a detail in
// which the two kernels differ and that shows in the instructions (which register array, which buffer descriptor, a scalar
// against a lane offset) is a compile-time parameter of the helper, never a silent unification - neither kernel is moved onto
// the other's form, and tools/device_code_same.py says whether that held.
#pragma once
#include "persist_common.h"

// ------------------------------------------------------------------------------------------ host
#define FRONT_MAX_LAYERS 8

// the padded width of the x panel (the kernels' FS) for a state size, 0 = no instantiation; the fronts take every frame
// size fs % 8 == 0 with 8 <= fs <= this width
static inline int front_panel(int S) { return S == 1024 ? 256 : S == 128 ? 64 : 0; }
static inline bool front_fs_ok(int S, int fs) { return fs >= 8 && fs % 8 == 0 && fs <= front_panel(S); }

// The first check of every front launcher: the caller's struct is this library's struct.
template <class A>
static int front_struct_ok(const char* who, const A* a, const char* type_name) {
  AG_REQUIRE(a && a->struct_bytes == (int64_t)sizeof(A), "%s: struct_bytes = %lld, but %s has %zu bytes in this library",
             who, a ? (long long)a->struct_bytes : -1LL, type_name, sizeof(A));
  return AG_OK;
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

// The per-layer tables of the stacked fronts (FRONT_MAX_LAYERS pointers per field): entry [l] of layer l's fields; `used`
// is the rule for a layer l < nl, and past nl every entry must be NULL.
template <int N>
static int front_layer_fields_ok(const char* who, int l, int nl, const FrontField (&f)[N]) {
  static const char* const idx[FRONT_MAX_LAYERS] = {"[0]", "[1]", "[2]", "[3]", "[4]", "[5]", "[6]", "[7]"};
  const bool in = l < nl;
  for (const FrontField& e : f) {
    const bool used = in && e.used;
    AG_REQUIRE((e.p != nullptr) == used, "%s: %s%s %s", who, e.name, idx[l],
               used ? "is NULL" : (in ? "is not used by this layer / mode and must be NULL" : "lies past nl and must be NULL"));
  }
  return AG_OK;
}

// ------------------------------------------------------------------------------------------ device: generation mode
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

// ------------------------------------------------------------------------------------------ device
// The one block of the frame loops that both forward kernels call.  The others that gfront_stack_*_kernel took over from
// gfront_persist_*_kernel are still spelled out in both files: moved into a helper they changed the instructions of the
// kernels around them, or could replace only some of their copies (profiles/front_parts_isa.txt has the list).  A helper
// is inlined only after the compiler has simplified helper and kernel separately, so a branch, a run-time loop or index
// arithmetic that crosses that boundary re-orders the code around it.

// a wave's 32x32 gate accumulator -> its slice of red [8 waves][1024]
__device__ __forceinline__ void front_acc_to_red(float* red, int wid, int lane, f32x16 acc) {
#pragma unroll
  for (int e = 0; e < 16; ++e) red[wid * 1024 + e * 64 + lane] = acc[e];
}

/* audiogan_hip.h  --  C ABI of libaudiogan_hip.so (gfx950 / MI355X only).
 *
 * The reference (BarclayII/audiogan) has no FFI layer: its hot path bottoms out in
 * third-party PyTorch ops called from audiogan.py.  Each entry point below replaces
 * one of those implicit device ops; the comment on each names the reference call
 * site(s) it stands in for (paths relative to /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless its name ends in _i64
 *     (int64) or says otherwise; the library borrows them for the call and owns
 *     nothing except the descriptor tables it is handed.
 *   - tensors are dense along their last (time / feature) axis; batch and channel
 *     strides are passed explicitly (in elements) so a layer can read from / write
 *     into a slice of a pre-allocated channel slab (this is what removes the
 *     T.cat at audiogan.py:467).
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never
 *     synchronised.  No allocation, no host sync inside any call (graph-capturable).
 *   - return value: AG_OK (0) or a negative AG_ERR_* code; never aborts.
 */
#ifndef AUDIOGAN_HIP_H
#define AUDIOGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AG_OK 0
#define AG_ERR_ARG (-1)         /* bad shape / null pointer / unsupported size     */
#define AG_ERR_LAUNCH (-2)      /* hipGetLastError() != hipSuccess after a launch  */
#define AG_ERR_UNSUPPORTED (-3) /* valid request this build has no kernel for      */

#define AG_ACT_NONE 0
#define AG_ACT_LEAKY 1 /* LeakyReLU(slope): audiogan.py:261,277,532 (slope 0.01) */
#define AG_ACT_TANH 2  /* audiogan.py:443 */
/* ag_conv1d_engine only: `res` is not a residual but the SAVED OUTPUT y of a LeakyReLU; the result is scaled by that
 * activation's derivative (1 where y > 0, slope elsewhere) - the LeakyReLU backward of the layer below folded into this
 * layer's backward-data pass (the .backward() of audiogan.py:277, :532); bias, length mask and accumulate as usual */
#define AG_ACT_LEAKY_GATE 3

/* library / build identification (ABI version, gfx arch string) */
int ag_abi_version(void);
const char* ag_arch(void);
const char* ag_last_error(void);
/* Name of the compute kernel that the calling thread's most recent call to ag_gemm, ag_gemm_h, ag_conv1d_engine or
 * ag_conv1d_wgrad (the entry points that choose among kernel forms) launched, as rocprofv3 spells it without the leading
 * "void ", the parameter list and spaces: "conv_engine_kernel<2,1,2,2,7,2>", "gemm_bf16_kernel<0,1,0>".  "" before the
 * first such call on this thread; a call that fails before its launch leaves the previous name.  Per thread, like
 * ag_last_error: read it on the thread that made the call (backward calls come from the autograd thread).
 * The name is recorded at the launch site itself, from the template arguments of the launch.  A call with several launches
 * is named after its main product: second stages (the slab / split-K reduces) record no name, and a transposed conv that
 * adds a tail launch for its ragged last columns puts the main launch's name back after the tail.  The string is static
 * storage owned by the library. */
const char* ag_last_kernel(void);

/* ---------------------------------------------------------------------------
 * Weight norm  (audiogan.py:77-80; torch.nn.utils.weight_norm, dim 0)
 *   w[r, :] = g[r] * v[r, :] / ||v[r, :]||_2      rows = size of dim 0, cols = rest
 * A table of `n` descriptors (device memory, see ag_wn_desc) is processed by ONE
 * launch.  For 3-D conv weights the kernel can also emit the two MFMA-friendly
 * layouts the conv engine consumes (see ag_conv1d_engine).
 * ------------------------------------------------------------------------- */
typedef struct ag_wn_desc {
  const float* v;  /* [rows, cols]                                      */
  const float* g;  /* [rows]                                            */
  float* w;        /* [rows, cols] standard layout (may be NULL)        */
  float* wpa;      /* gather layout  [pad2(d1)][K][pad32(d0)]  or NULL  */
  float* wpb;      /* scatter layout [d0][ceil(K/s)][pad32(d1*s)] or NULL */
                   /* Each layout [Cp2][taps][rows] is followed IN THE SAME BUFFER by its bf16 image
                    * [ceil(Cp2/16)][taps][2][rows][8 x bf16] (what the bf16-MFMA conv kernel stages in AG_PREC_BF16
                    * mode); ag_wpa_numel / ag_wpb_numel return the size of both parts, the buffers must start
                    * zero-filled (padding is never written).                                                  */
  float* inv_norm; /* [rows] 1/||v||, saved for backward (may be NULL)  */
  int32_t rows;    /* d0                                                */
  int32_t cols;    /* d1*K                                              */
  int32_t d1;      /* second dim (1 for 2-D / 1-D tensors)              */
  int32_t K;       /* taps (1 for 2-D / 1-D tensors)                    */
  int32_t stride;  /* conv stride used for the wpb layout               */
  int32_t pad;     /* conv padding the wpb layout is prepared for: when pad % stride != 0 and it costs no tap slot,
                    * phase r's taps sit ceil(pad/s) - ceil((pad-r)/s) slots later ("aligned" layout, see
                    * ag_conv_args.wp_pad); 0 = plain layout */
} ag_wn_desc;

int ag_weight_norm_fwd(const ag_wn_desc* descs_dev, int n, int max_rows, void* stream);

typedef struct ag_wn_bwd_desc {
  const float* v;
  const float* g;
  const float* dw; /* [rows, cols] gradient wrt w (standard layout) */
  float* dv;       /* [rows, cols] */
  float* dg;       /* [rows] */
  int32_t rows;
  int32_t cols;
  int32_t accumulate; /* 1: dv += ..., dg += ... (gradient accumulation straight into .grad) */
  int32_t pad_;
} ag_wn_bwd_desc;

int ag_weight_norm_bwd(const ag_wn_bwd_desc* descs_dev, int n, int max_rows, void* stream);

/* ---------------------------------------------------------------------------
 * 1-D convolution engine (fp32 MFMA implicit GEMM).  One kernel family covers
 *   mode 0 "gather":  y[b,o,t]      = sum_{c,k} W[o,c,k] x[b,c, s*t+k-p]
 *        = NN.Conv1d forward            (audiogan.py:272,406,490)
 *        = NN.ConvTranspose1d backward-data
 *   mode 1 "scatter": y[b,o,s*t+k-p] += sum_c W[c,o,k] x[b,c,t]
 *        = NN.ConvTranspose1d forward   (audiogan.py:275)
 *        = NN.Conv1d backward-data      (loss.backward(), audiogan.py:785,903)
 * followed by the fused epilogue
 *   v = acc + bias[o] + res[b,o,t];  v = act(v);  v *= (t < lens_i64[b]);
 *   y = accumulate ? y + v : v
 * (bias/res/lens optional).  `wp` is the prepared weight layout written by
 * ag_weight_norm_fwd (wpa for mode 0, wpb for mode 1) or by ag_prep_conv_weight.
 * ------------------------------------------------------------------------- */
typedef struct ag_conv_args {
  const float* x;
  const float* wp;
  const float* bias;
  const float* res;
  float* y;
  const int64_t* lens_i64;
  int64_t x_bs, x_cs;     /* input batch / channel stride (elements)  */
  int64_t y_bs, y_cs;     /* output strides                            */
  int64_t res_bs, res_cs; /* residual strides                          */
  int32_t B, C, Lin, O, Lout;
  int32_t K, stride, pad; /* parameters of the underlying conv         */
  int32_t mode;           /* 0 gather, 1 scatter                       */
  int32_t act;            /* AG_ACT_*                                  */
  float slope;
  int32_t accumulate;
  int32_t wp_pad;         /* mode 1: the padding `wp` was prepared for (ag_wn_desc.pad / ag_prep_conv_weight's pad).
                           * Equal to `pad` with pad % stride != 0: the aligned scatter layout is assumed and all
                           * phases share one column range (no ragged last column); anything else: plain layout */
} ag_conv_args;

int ag_conv1d_engine(const ag_conv_args* args, void* stream);

/* plain (non weight-normed) weights -> engine layouts; w is [d0][d1][K] */
int ag_prep_conv_weight(const float* w, float* wpa, float* wpb, int d0, int d1, int K, int stride, int pad,
                        void* stream);
/* sizes (in floats) of the two layouts - fp32 part + bf16 image, see ag_wn_desc - so the host can allocate them */
int64_t ag_wpa_numel(int d0, int d1, int K);
int64_t ag_wpb_numel(int d0, int d1, int K, int stride);

/* Weight gradient of a strided conv (conv backward-weight, convT backward-weight):
 *   dw[a,c,k] (+)= sum_{b,t} sh[b,a,t] * lg[b,c, s*t+k-p]
 * Conv1d:          sh = dY (a = out ch),  lg = x  (c = in ch)   -> dw[O][C][K]
 * ConvTranspose1d: sh = x  (a = in ch),   lg = dY (c = out ch)  -> dw[Ci][Co][K]
 * dw must be zero-filled (or hold a value to accumulate into); fp32 atomics. */
int ag_conv1d_wgrad(const float* sh, int64_t sh_bs, int64_t sh_cs, const float* lg, int64_t lg_bs,
                    int64_t lg_cs, float* dw, int B, int A, int Lsh, int C, int Llg, int K,
                    int stride, int pad, void* stream);

/* Single-output-channel stride-1 'same' convolution (the Generator's final Conv1d 113 -> 1, k3,
 * audiogan.py:404-407): one output channel cannot fill an MFMA tile and the layer is HBM-bound, so it
 * has plain vector kernels.  w is the standard [1, C, K] weight (= [C, K]); K <= 9.
 *   fwd      y[b,t]      = act(bias + sum_{c,k} w[c,k] x[b,c,t+k-pad])
 *   bwd_data dx[b,c,t] (+)= sum_k w[c,k] dy[b,t-k+pad]
 *   wgrad    dw[c,k]    += sum_{b,t} dy[b,t] x[b,c,t+k-pad]        (two-stage, needs a bound workspace; dw pre-zeroed) */
int ag_conv1d_o1_fwd(const float* x, int64_t x_bs, int64_t x_cs, const float* w, const float* bias, float* y,
                     int64_t y_bs, int B, int C, int L, int K, int pad, int act, float slope, void* stream);
int ag_conv1d_o1_bwd_data(const float* dy, int64_t dy_bs, const float* w, float* dx, int64_t dx_bs,
                          int64_t dx_cs, int B, int C, int L, int K, int pad, int accumulate, void* stream);
int ag_conv1d_o1_wgrad(const float* dy, int64_t dy_bs, const float* x, int64_t x_bs, int64_t x_cs, float* dw,
                       int B, int C, int L, int K, int pad, void* stream);

/* db[c] = (accumulate ? db[c] : 0) + sum_{b,t} dy[b,c,t]   (bias gradient; two-stage through the bound workspace) */
int ag_channel_sum(const float* dy, int64_t bs, int64_t cs, float* db, int B, int C, int L, int accumulate,
                   void* stream);

/* dpre = dy * (y > 0 ? 1 : slope) * (t < lens[b])   elementwise on [B,C,L] views.
 * LeakyReLU keeps the sign, so the saved OUTPUT y is enough (no pre-activation).
 * add_into (optional, same shape): add_into += dpre  -- the gradient of the
 * "act += x[:, -out:, :]" skip connection of dense_res_bottleneck (audiogan.py:281-282).
 * bias_grad (optional, [C]): bias_grad[c] += sum_{b,t} dpre[b,c,t] -- the bias gradient of the conv that
 * produced y, taken in the same pass (atomics; pre-zeroed by the caller). */
int ag_leaky_bwd(const float* dy, int64_t dy_bs, int64_t dy_cs, const float* y, int64_t y_bs,
                 int64_t y_cs, float* dpre, int64_t dp_bs, int64_t dp_cs, float* add_into,
                 int64_t ad_bs, int64_t ad_cs, const int64_t* lens_i64, float* bias_grad, int B, int C,
                 int L, float slope, void* stream);

/* ---------------------------------------------------------------------------
 * Dense fp32 GEMM on MFMA (NN.Linear / LSTM gate products: audiogan.py:260,380,
 * 385,409,410,498,509,511 and their backward):
 *   C[M,N] = act( alpha * op(A)[M,K] * op(B)[K,N] + beta * C + bias[N] + res[M,N] )
 * ta: 0 -> A is [M,K] row-major (lda), 1 -> A is stored [K,M]
 * tb: 0 -> B is [K,N] row-major (ldb), 1 -> B is stored [N,K]   (Linear weight)
 * act = AG_ACT_LEAKY_GATE: `res` is not added; it is the saved OUTPUT of a LeakyReLU and the result is scaled by that
 * LeakyReLU's derivative (1 where res > 0, slope elsewhere): the activation backward of the heads (audiogan.py:261,:510
 * under .backward()) rides in the epilogue of the backward-data product.
 * ------------------------------------------------------------------------- */
int ag_gemm(const float* A, int lda, int ta, const float* B, int ldb, int tb, float* C, int ldc,
            int M, int N, int K, float alpha, float beta, const float* bias, const float* res,
            int ldres, int act, float slope, void* stream);

/* column sums: out[n] = (accumulate ? out[n] : 0) + sum_m X[m, n]   (Linear bias gradient; two-stage through the bound
 * workspace, or one row block per column when none is bound) */
int ag_col_sum(const void* X, int x_bf16 /* X stored as bfloat16, ldx in 2-byte elements */, int ldx, float* out, int M, int N,
               int accumulate, void* stream);

/* ---------------------------------------------------------------------------
 * LSTM cell pointwise step (NN.LSTMCell / NN.LSTM, audiogan.py:380,440-442,498):
 * gates[B,4H] hold i|f|g|o pre-activations (PyTorch order) INCLUDING biases.
 *   i,f,o = sigmoid, g = tanh;  c' = f*c + i*g;  h' = o*tanh(c')
 * fwd overwrites gates with the ACTIVATED values (saved for backward).
 * `valid_i64`/`t`: rows with t >= valid[b] keep (h,c) unchanged and output 0
 * (packed-sequence semantics of dynamic_rnn, audiogan.py:214-229); NULL = all valid.
 * ------------------------------------------------------------------------- */
int ag_lstm_cell_fwd(float* gates, int ldg, const float* c_prev, int ldcp, float* h_out, int ldh,
                     float* c_out, int ldc, float* y_out, int ldy, const float* h_prev, int ldhp,
                     const int64_t* valid_i64, int t, int B, int H, void* stream);
/* backward: dh = gradient reaching the state h' from later steps (NULL = 0), dy = gradient
 * of the step's output (NULL = 0), dc_next (NULL = 0) -> dgates (pre-activation), dc_prev.
 * Valid rows use dh + dy and write dh_pass = 0; padded rows write dgates = 0,
 * dc_prev = dc_next and pass dh through (dh_pass = dh; their output was the constant 0). */
int ag_lstm_cell_bwd(const float* gates_act, int ldg, const float* c_prev, int ldcp,
                     const float* c_new, int ldc, const float* dh, int lddh, const float* dy,
                     int lddy, const float* dc_next, int lddcn, float* dgates, int lddg,
                     float* dc_prev, int lddcp, float* dh_pass, int lddhp, const int64_t* valid_i64,
                     int t, int B, int H, void* stream);

/* GRU cell pointwise step (BASELINE config C4; the reference has no GRU -- SURVEY.md F5 -- so the
 * contract is torch.nn.GRUCell's: gate order r|z|n, n = tanh(gi_n + r * gh_n)).  gi [B,3H] and
 * gh [B,3H] (contiguous) hold the complete input / hidden products incl. biases; fwd overwrites gi
 * with the activated (r,z,n), gh keeps gh_n.  bwd writes dgi, dgh and dh_prev = dh * z. */
int ag_gru_cell_fwd(float* gi, const float* gh, const float* h_prev, int ldhp, float* h_out, int ldh,
                    int B, int H, void* stream);
int ag_gru_cell_bwd(const float* gates_act, const float* gh, const float* h_prev, int ldhp,
                    const float* dh, int lddh, float* dgi, float* dgh, float* dh_prev, int lddhp, int B,
                    int H, void* stream);

/* Precision mode of every contraction launched by this PROCESS from now on (default 0 = fp32; process-wide because
 * an autograd engine runs backward passes on a thread of its own).
 *   1 = bf16: each contraction (conv / transposed conv / linear / recurrent products, in their forward,
 *   backward-data and backward-weight forms) rounds BOTH operands to bfloat16 (round-to-nearest-even) and accumulates in
 *   fp32; tensors in memory, epilogues, losses and the optimiser stay fp32.  ag_gemm and the persistent recurrent
 *   kernels run v_mfma_f32_32x32x16_bf16 in this mode; the other kernels round their operands in registers in front of
 *   the fp32 MFMA (same sums up to the order of the fp32 additions).  Spec: BASELINE.json configs[2] (bf16, 8 GPUs);
 *   the reference itself is fp32 only. */
#define AG_PREC_F32 0
#define AG_PREC_BF16 1
/*   2 = f32x3, an EXPERIMENT (bench.py --dtype f32x3; never the headline precision): the large ag_gemm products (128x128-tile
 *   class) split both operands into bfloat16 hi + lo parts and sum hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32
 *   accumulation (~2^-16 relative per product); every other kernel computes exactly as in mode 0. */
#define AG_PREC_F32X3 2
int ag_set_precision(int mode);
int ag_get_precision(void);

/* Deterministic cross-workgroup reductions.  Entry points that sum over workgroups (ag_conv1d_wgrad,
 * ag_conv1d_o1_wgrad, ag_channel_sum, ag_leaky_bwd's bias gradient, ag_gemm's split-K products, ag_col_sum,
 * ag_skinny_gemm in accumulate mode, ag_lstm_seq_bwd's unfused fallback, ag_grad_norms) do so in TWO STAGES through a
 * bound workspace: partial results with plain stores, then a sum in a fixed order - bitwise reproducible.  There is NO
 * float-atomic path any more (round 4): a call whose sum spans workgroups returns AG_ERR_ARG when no (or too small a)
 * workspace is bound; ag_gemm and ag_col_sum then run unsplit instead.  ag_bind_workspace() binds `numel` floats (16-byte
 * aligned device memory on the launch stream's device) for the NEXT such call of this host thread; the call consumes
 * the binding.  The ag_*_ws_numel() functions return the size a call wants (0: none needed); a smaller workspace (down to
 * the minimum each call states in its error text) reduces the number of partial slabs. */
int ag_bind_workspace(float* ws, int64_t numel);
int64_t ag_conv1d_wgrad_ws_numel(int B, int A, int Lsh, int C, int K);
int64_t ag_gemm_ws_numel(int M, int N, int K, int act);

/* Batched 2-D transpose through LDS: out[b][j][i] = in[b][i][j] for i < R, j < Cc; in element (b,i,j) at in + b*ibs + i*irs + j,
 * out element (b,j,i) at out + b*obs + j*ors + i (inner index contiguous on both sides).  The critic's conv features
 * [B,C,T'] -> time-major [T',B,C] for the biLSTM (audiogan.py:542) and the gradient's way back. */
/* (round 4) in_bf16 / out_bf16: that side is stored as bfloat16 (strides in elements of its own type; fp32 -> bf16 rounds to
 * nearest even): in AG_PREC_BF16 mode with bf16 storage the time-major features are written as bf16, the operand type of
 * ag_gemm_h, and their gradient comes back as bf16 */
int ag_transpose_batched(const void* in, int in_bf16, int64_t ibs, int64_t irs, void* out, int out_bf16, int64_t obs,
                         int64_t ors, int B, int R, int Cc, void* stream);

/* Input assembly, one launch each (round 4; replaces T.cat / expand / transpose / + on the iteration path).
 * ag_build_zc: zc[t,b,:] = [z[b,t,:ns] | c[b,:es]], the non-recurrent part of the Generator front's LSTM input
 * (audiogan.py:433-439: z [B,T,ns], c [B,es] -> zc [T,B,ns+es] contiguous).
 * ag_critic_batch: the critic's minibatch (audiogan.py:724-728, :749-751, :844): rows [0,nA) = xa + na, rows [nA,nA+nB) =
 * xb + nb (na / nb = instance noise, NULL = none; row pitches in elements) -> x_out [nA+nB, L] contiguous; the rows'
 * lengths after every conv layer, lens_out[i, row] = ceil(len / prods[i]) (audiogan.py:533; lenA / lenB NULL = L; prods =
 * the nl <= 8 cumulative stride products, a HOST array) and the conditioning rows c_out = [cA ; cB] ([.,E]; NULL = skip). */
/* A Linear layer with ONE output (the critic's last layer 512 -> 1, audiogan.py:511,:549; the Generator's stop head
 * 1024 -> 1, :410,:445).  ag_rowdot_fwd: y[m*ldy] = x[m,:K] . w + bias[0] (bias may be NULL).  ag_rowdot_bwd, one pass over
 * x: dx[m,k] = dy[m*lddy] * w[k] (times LeakyReLU'(x[m,k]) when gate: x is then the SAVED OUTPUT of the LeakyReLU below;
 * dx may be NULL), and when dw != NULL: dw[k] (+)= sum_m dy[m] x[m,k], db[0] (+)= sum_m dy[m] with db == dw + K (one
 * [K+1] gradient row), two-stage through a bound workspace of ag_rowdot_bwd_ws_numel floats (deferrable).
 * x_bf16 / h16: x (and dx) are stored as bfloat16, pitches in 2-byte elements (the bf16-storage path of AG_PREC_BF16). */
int ag_rowdot_fwd(const void* x, int x_bf16, int ldx, const float* w, const float* bias, float* y, int64_t ldy, int M, int K,
                  void* stream);
int64_t ag_rowdot_bwd_ws_numel(int M, int K);
int ag_rowdot_bwd(const float* dy, int64_t lddy, const void* x, int ldx, const float* w, void* dx, int lddx, int h16, float* dw,
                  float* db, int accumulate, int M, int K, int gate, float slope, void* stream);
int ag_build_zc(const float* z, const float* c, float* zc, int B, int T, int ns, int es, void* stream);

/* ---------------------------------------------------------------------------
 * GEMM on operands STORED as bfloat16 (BASELINE configs[2]; csrc/gemm_bf16s.hip):
 *   C[M,N] = act(alpha * op(A) op(B) + beta * C + bias + res), fp32 accumulation, output as fp32 (C) and / or bf16 (C16)
 * A / B: bfloat16 bit patterns; ta / tb as ag_gemm.  Tiles go global -> LDS by LDS-DMA (no convert, half the bytes of the
 * fp32-operand kernel); k-strided operands (ta = 1, tb = 0: weight gradients, the weight of a data gradient) are read
 * with the transposed LDS read of gfx950.  res (fp32) or res16 (bf16): residual, or with AG_ACT_LEAKY_GATE the saved
 * activation whose derivative scales the result; gate16 (bf16, optional): a saved LeakyReLU output applied AFTER bias /
 * res (a residual layer's backward: (W^T da + da) gated by the layer below).  Shapes: ag_gemm_h_ok (K % 64 == 0, leading
 * dimensions % 8 == 0, row counts % 8 == 0 for k-strided operands, 16-byte aligned operands).  Split-K (fp32 output, plain
 * epilogue) through a bound workspace of ag_gemm_h_ws_numel floats; its second stage is deferrable.  A product with a
 * bf16 residual runs unsplit (the second stage adds fp32 residuals only); a workspace bound for it is left unused.
 * ag_to_bf16_2d: dst[r,c] = bf16(src[r,c]) for a pitched [rows <= 65535, cols] block (weights -> their bf16 image).
 * ------------------------------------------------------------------------- */
int ag_gemm_h_ok(int M, int N, int K, int ta, int tb, int lda, int ldb);
int64_t ag_gemm_h_ws_numel(int M, int N, int K, int act, int has_c16);
int ag_gemm_h(const uint16_t* A, int lda, int ta, const uint16_t* B, int ldb, int tb, float* C, int ldc, uint16_t* C16,
              int ldc16, int M, int N, int K, float alpha, float beta, const float* bias, const float* res, int ldres,
              const uint16_t* res16, int ldres16, const uint16_t* gate16, int ldgate16, int act, float slope, void* stream);
int ag_to_bf16_2d(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int rows, int cols, void* stream);
int ag_critic_batch(const float* xa, int64_t xa_ld, const float* na, int64_t na_ld, int nA, const float* xb,
                    int64_t xb_ld, const float* nb, int64_t nb_ld, int nB, int L, float* x_out,
                    const int64_t* lenA_i64, const int64_t* lenB_i64, const int32_t* prods_host, int nl,
                    int64_t* lens_out_i64, const float* cA, const float* cB, int E, float* c_out, void* stream);

/* Deferred second stages.  Between ag_defer_reduces(1) and ag_flush_reduces() every two-stage reduction (conv weight
 * gradients, bias / channel / column sums, and a split-K ag_gemm whose second stage has a plain epilogue: contiguous C, no
 * bias / res, beta 0 or 1) only records its second stage; the flush sums all recorded outputs in ONE launch, each in the
 * order its own launch would use (bitwise the same results).  The caller keeps every bound workspace alive until the flush
 * and turns deferral off again with ag_defer_reduces(0) (an error if recorded stages were never flushed).
 * Modes: 1 = start recording, 0 = stop, 2 = pause (a call issued now finishes at once; recorded stages stay), 3 = resume.
 * Process-wide since round 4 (a scope is opened by the thread that calls backward(), the recording calls come from
 * torch's autograd thread; never concurrently), unlike ag_bind_workspace, which stays per thread. */
int ag_defer_reduces(int mode);
int ag_flush_reduces(void* stream);
int64_t ag_skinny_ws_numel(int M, int N, int K);

/* Skinny product for the sequential part of the recurrent layers (M = clips per call <= 256):
 *   C[M,N] = act(A[M,K] * op(B) + beta*C + bias)         (accumulate_atomic == 0)
 *   C[M,N] += A[M,K] * op(B) (+ bias)   K split over workgroups, fp32 atomics  (== 1)
 * tb: 1 -> B stored [N,K] (Linear weight), 0 -> B stored [K,N].  Needs K % 8 == 0 and 16-byte
 * aligned rows of A (and of B when tb == 1). */
int ag_skinny_gemm(const float* A, int lda, const float* B, int ldb, int tb, float* C, int ldc,
                   int M, int N, int K, float beta, const float* bias, int act, float slope,
                   int accumulate_atomic, void* stream);

/* One fused LSTMCell step (audiogan.py:439-442): gates_pre [B,4H] holds the part of the gate
 * pre-activations that does not depend on the recurrence (z/c columns of W_ih + both biases);
 * the kernel adds x[B,Kx]*wx^T (fed-back frame, columns [0,Kx) of W_ih) and h_prev*whh^T,
 * applies the cell and overwrites gates_pre with the activated gates. first_step: x and h_prev
 * are zero and skipped. */
int ag_lstm_step_fwd(float* gates_pre, const float* x, int ldx, const float* wx, int ldwx, int Kx,
                     const float* h_prev, const float* whh, const float* c_prev, float* c_out,
                     float* h_out, int B, int H, int first_step, void* stream);

/* A whole (bi)directional NN.LSTM layer over a padded batch (audiogan.py:498-503, :543 and the
 * pack/unpack of :214-229 expressed as a per-clip valid length): T fused steps enqueued by one
 * call.  Tables are HOST arrays of device pointers, one entry per direction.
 *   pre[d]   [T,B,4H] x-projection + biases; overwritten with the activated gates
 *   whh[d]   [4H,H];  c_all[d] [T+1,B,H] with c_all[d][0] = 0;  hbuf[d] [2,B,H] scratch
 *   y        [T,B,ndir*H]; direction 1 walks the sequence backwards
 *   static_pre  NULL, or a table of [B,4H] tensors added to the pre-activations of EVERY step: the projection of
 *            a time-invariant part of the input (the Discriminator concatenates the conditioning vector c to
 *            every frame, audiogan.py:541) plus the biases - computed once per clip instead of once per frame
 * Processing steps [k_begin, k_end) are enqueued (0, T for the whole layer; the state buffers
 * carry over between calls, forward in increasing and backward in decreasing step order).
 * ag_lstm_seq_bwd's `phases` is 3 in normal use; 1 enqueues only the pointwise cell backward and
 * 2 only the recurrent product of each step (lets a profiler time the two kernels separately). */
int ag_lstm_seq_fwd(float* const* pre, const float* const* whh, float* const* c_all,
                    float* const* hbuf, float* y, const int64_t* valid_i64, const float* const* static_pre,
                    int T, int B, int H, int ndir, int k_begin, int k_end, void* stream);
int ag_lstm_seq_bwd(const float* const* gates, const float* const* whh, const float* const* c_all,
                    const float* dy, float* const* dgates, float* const* dhbuf, float* const* dcbuf,
                    const int64_t* valid_i64, int T, int B, int H, int ndir, int k_begin, int k_end,
                    int phases, void* stream);

/* The same layer forward as ONE persistent launch with W_hh resident in LDS (csrc/lstm_persist.hip): each
 * workgroup owns 8 hidden units x 32 or 64 clips of one direction for the whole sequence; only the hidden state
 * crosses workgroups (write-through stores + one agent-scope flag per workgroup and step).  Replaces T launches
 * that re-stream W_hh from the fabric each.  Needs every workgroup co-resident: ag_lstm_persist_ok() says whether
 * (B, H, ndir) fits `n_cu` compute units (H % 64 == 0, H <= 768, ndir * ceil(B/32 or 64) * H/8 <= n_cu); `ws` is
 * ag_lstm_persist_ws_bytes() bytes of 16-byte aligned device memory owned by this launch while it is in flight.
 * Workspace layout: [256 B sticky area][8 KiB header: launch status + flags][exchange buffers].  The header is zeroed
 * by a memset node enqueued in front of the kernel.  The STICKY word (word 0 of the workspace, zero when the caller
 * allocates it) is never cleared by a launch: every bounded spin that times out ORs 0x80000000|step into it, so one
 * host read after any number of launches tells whether all of them completed.  A
 * workgroup that gave up writes NaN into everything it produces from then on, so the failure also reaches the loss.
 * ONE persistent launch per device at a time.
 * Tensors as for ag_lstm_seq_fwd (no hbuf: the state stays in registers). */
/* test hook, ONE-SHOT and per thread: timeout of the bounded spins in ticks of the 100 MHz realtime counter (<= 0: the
 * default 3 s) and one block index that never publishes its flags (-1: none), applied to the NEXT persistent launch the
 * calling thread enqueues and consumed by it (every later launch runs with the defaults again) */
int ag_persist_debug(int64_t timeout_ticks, int mute_block);
int ag_lstm_persist_ok(int B, int H, int ndir, int n_cu);
int64_t ag_lstm_persist_ws_bytes(int B, int H, int ndir);
/* (round 4) y_bf16: the layer output y is WRITTEN as bfloat16 (y then addresses 2-byte elements) - the operand type of the
 * products that consume it (ag_gemm_h) */
int ag_lstm_seq_fwd_persist(float* const* pre, const float* const* whh, float* const* c_all, void* y, int y_bf16,
                            const int64_t* valid_i64, const float* const* static_pre, void* ws, int64_t ws_bytes,
                            int T, int B, int H, int ndir, int n_cu, void* stream);

/* The layer's backward through time as ONE persistent launch: each workgroup (16 clips x 32 hidden units of one
 * direction) keeps its [4H x 32] panel of W_hh in REGISTERS for the whole sequence; dgates_k is written through
 * into the output tensor, which doubles as the exchange buffer.  H in {64,128,256,512} and
 * ndir * ceil(B/16) * H/32 <= n_cu (ag_lstm_persist_bwd_ok); `ws` >= 256 B + 8 KiB, laid out as above.  Tensors as for
 * ag_lstm_seq_bwd (no dhbuf/dcbuf: the state stays in registers). */
int ag_lstm_persist_bwd_ok(int B, int H, int ndir, int n_cu);
/* (round 4) dy_bf16: dy is stored as bfloat16; dg16: optional table of ndir [T,B,4H] bfloat16 outputs, dgates rounded - the
 * operand type of ag_gemm_h for the weight / input gradient products (dgates itself stays fp32: it is the exchange buffer).
 * dgsum: optional table of ndir [B,4H] outputs, the sum over time of dgates (what the biases and a time-invariant
 * input see), accumulated in registers by the thread that produces each (clip, gate) pair - no separate pass over dgates */
int ag_lstm_seq_bwd_persist(const float* const* gates, const float* const* whh, const float* const* c_all,
                            const void* dy, int dy_bf16, float* const* dgates, float* const* dgsum, uint16_t* const* dg16,
                            int dg16_ld /* row pitch of dg16 in elements, >= 4H */, const int64_t* valid_i64, void* ws,
                            int64_t ws_bytes, int T, int B, int H, int ndir, int n_cu, void* stream);

/* The Generator front's whole frame loop (audiogan.py:428-460: one recurrent cell + tanh(proj) fed back) as ONE
 * persistent launch with every weight resident in registers (csrc/front_persist.hip), in two modes:
 *   training (gen 0): `gates` comes in as the z / c part of the pre-activations (one GEMM over all frames) and goes out
 *     activated; the history the backward needs (hs, cs or gh, xt) is written beside the frames x.
 *   generation (gen 1, Generator.generate): the frame loop of a SAMPLE, trains nothing and keeps no history - `gates` is only
 *     read and only x is written.  Per frame the launch also forms the stop logit s[b,t] = h_t[b] . w_s + b_s and draws
 *     stop[b,t] = u[t,b] < sigmoid(s[b,t]) from the caller's uniforms (audiogan.py:444-460: a Bernoulli(p) draw, stated as a
 *     function of u so that it can be reproduced).  The loop ends early, by one rule every workgroup takes from the same
 *     write-once words: before frame t + 1 it reads the decisions of frame t - 1 (a lag of one frame) and leaves iff every
 *     clip has stopped by then, so t_run = min(T, max(first) + 1).  Frames past max(first) are correct frames the caller
 *     discards; x and s are written for the frames run only.
 * and with two cells: 0 = LSTMCell (G = 4 gate blocks i f g o), 1 = GRU cell (BASELINE configs[3]: the LSTMCell of :380-386
 * replaced by a GRU cell; G = 3, gate order r z n as torch.nn.GRUCell).
 * Supported (ag_gfront_persist_ok): S = 1024 with any frame size fs % 8 == 0, 8 <= fs <= 256 (the reference's default 200
 * among them), S = 128 with fs % 8 == 0, 8 <= fs <= 64; B <= 64 and ceil(B/32) * S/8 <= n_cu.  The kernels keep the x panel
 * at the padded width 256 / 64: lanes at or past fs hold zeros, rows of x have the pitch fs (in generation mode the stop
 * workgroups are those of column tile 0, which every fs has).  `ws` = ag_gfront_persist_ws_bytes() bytes (sized for the
 * padded width: the same for every fs of a state size), used as for ag_lstm_seq_fwd_persist.
 *
 * Every tensor is fp32 and dense in the stated shape unless a pitch (in elements) is named; w_x, w_hh, w_p and `ws` are
 * 16-byte aligned, ldwx % 4 == 0.  A field that the chosen (cell, gen) does not use must be NULL. */
typedef struct ag_front_fwd_args {
  int64_t struct_bytes; /* sizeof(ag_front_fwd_args): a caller built against another layout is refused */
  int32_t cell;         /* 0 LSTM, 1 GRU */
  int32_t gen;          /* 0 training, 1 generation */
  float* gates;         /* all: [T,B,G*S].  in: W_ih[:, fs:] zc_t + b_ih + (LSTM: b_hh; GRU: (b_hr, b_hz, 0));
                           training: out = activated gates; generation: only read */
  float* gh;            /* GRU training: [T,B,3S] out, only its n slot is written (W_hn h_{t-1} + b_hn, what the backward reads) */
  const float* w_x;     /* all: W_ih[:, :fs], [G*S,fs] with row pitch ldwx */
  const float* w_hh;    /* all: [G*S,S] */
  const float* b_hn;    /* GRU, both modes: [S] = b_hh[2S:] */
  const float* w_p;     /* all: [fs,S] */
  const float* b_p;     /* all: [fs] */
  float* hs;            /* training: [T,B,S] out, h_t */
  float* cs;            /* LSTM training: [T+1,B,S] out (cs[0] is written 0 by the launch) */
  float* x;             /* all: [B,T*fs] out, row pitch ldx: the caller may hand over channel 0 of the conv trunk's
                           activation slab, so the frames land where the trunk reads them (no copy) */
  float* xt;            /* training, optional: [T,B,fs] out, the same frames time-major (what the weight-gradient products read) */
  const float* w_s;     /* generation: [S], the materialised stop head */
  const float* b_s;     /* generation: [1] */
  const float* u;       /* generation: [T,B] uniforms */
  float* s;             /* generation: [B,T] out, row pitch lds >= T: the stop logits */
  int32_t* first;       /* generation: [B] out, the frames clip b generates (1 + its first stop frame, T if it never stops) */
  int32_t* t_run;       /* generation: [1] out, the frames run */
  void* ws;             /* all: the workspace */
  int64_t ldx, lds, ws_bytes;
  int32_t ldwx, T, B, S, fs, n_cu;
} ag_front_fwd_args;
int ag_gfront_persist_ok(int B, int S, int fs, int n_cu);
int64_t ag_gfront_persist_ws_bytes(int B, int S, int fs);
int ag_gfront_fwd(const ag_front_fwd_args* a, void* stream);

/* The frame loop of a STACKED front (audiogan.py:382-385, :441-442: nl LSTMCell layers, 2 <= nl <= 8, under one projection
 * and one stop head, both fed by the top layer's h) as ONE persistent launch (csrc/front_stack.hip), in the two modes of
 * ag_gfront_fwd.  Frame t: layer 0 takes [x_{t-1}, zc_t] and its own h_{0,t-1}; layer l >= 1 takes h_{l-1,t} and its own
 * h_{l,t-1}; x_t = tanh(h_{nl-1,t} W_p^T + b_p); (generation) s_t = h_{nl-1,t} . w_s + b_s, with the stop draws, the exit
 * rule and the outputs s, first, t_run exactly as ag_gfront_fwd states them.  LSTMCell only.  fp32 MFMA; in bf16 mode
 * (ag_set_precision) both operands of all three products are rounded in registers.
 * Supported (ag_gfront_stack_ok): 2 <= nl <= 8; (S, fs) as for ag_gfront_persist_ok; 1 <= B <= 64 and
 * nl * ceil(B/32) * S/8 <= min(n_cu, 256) workgroups (256 at the reference's B 32, S 1024, nl 2).  One layer is NOT this
 * launch's business: ag_gfront_stack_ok answers 0 for nl = 1, which stays on ag_gfront_fwd.  `ws` =
 * ag_gfront_stack_ws_bytes() bytes (one h exchange buffer more per layer; the same for every fs of a state size), used as
 * for ag_lstm_seq_fwd_persist.
 *
 * Every tensor is fp32 and dense in the stated shape unless a pitch (in elements) is named; every w_hh, w_in, w_p and `ws`
 * are 16-byte aligned, ldwx % 4 == 0.  The per-layer tables hold 8 entries: entries from nl on must be NULL, and so must a
 * field that the mode (or the layer) does not use.  All of that, a wrong struct_bytes and T <= 0 are refused with AG_ERR_ARG
 * before any HIP call; a shape outside the rule with AG_ERR_UNSUPPORTED. */
typedef struct ag_front_stack_args {
  int64_t struct_bytes; /* sizeof(ag_front_stack_args): a caller built against another layout is refused */
  int32_t gen;          /* 0 training, 1 generation */
  int32_t nl;           /* layers */
  float* gates[8];      /* [T,B,4S] each.  [0], both modes: in = W_ih_0[:, fs:] zc_t + b_ih_0 + b_hh_0; training: out = activated
                           gates; generation: only read.  [l >= 1], training only: out = activated gates (never read) */
  float* hs[8];         /* training: [T,B,S] out, h_{l,t} */
  float* cs[8];         /* training: [T+1,B,S] out (cs[l][0] is written 0 by the launch) */
  const float* w_hh[8]; /* both: [4S,S] */
  const float* w_in[8]; /* both.  [0]: W_ih_0[:, :fs], [4S,fs] with row pitch ldwx; [l >= 1]: W_ih_l [4S,S] */
  const float* bias[8]; /* both.  [0]: NULL (its biases are inside gates[0]); [l >= 1]: b_ih_l + b_hh_l, [4S] */
  const float* w_p;     /* both: [fs,S] */
  const float* b_p;     /* both: [fs] */
  float* x;             /* both: [B,T*fs] out, row pitch ldx (channel 0 of the conv trunk's slab, or dense) */
  float* xt;            /* training, optional: [T,B,fs] out, the same frames time-major */
  const float* w_s;     /* generation: [S], the materialised stop head */
  const float* b_s;     /* generation: [1] */
  const float* u;       /* generation: [T,B] uniforms */
  float* s;             /* generation: [B,T] out, row pitch lds >= T: the stop logits of the frames run */
  int32_t* first;       /* generation: [B] out, the frames clip b generates */
  int32_t* t_run;       /* generation: [1] out, the frames run */
  void* ws;             /* both: the workspace */
  int64_t ldx, lds, ws_bytes;
  int32_t ldwx, T, B, S, fs, n_cu;
} ag_front_stack_args;
int ag_gfront_stack_ok(int B, int S, int fs, int nl, int n_cu);
int64_t ag_gfront_stack_ws_bytes(int B, int S, int fs, int nl);
int ag_gfront_stack_fwd(const ag_front_stack_args* a, void* stream);

/* The frame loop of the front's BACKWARD through time (audiogan.py:437-443 under .backward() :903) in one persistent
 * launch: per frame gx_t = (dx_ext[t] + dgates_{t+1} W_x)(1 - x_t^2), dh_t = dh_ext[t] + dgates_{t+1} W_hh + gx_t W_p,
 * dgates_t = cell backward (cell 1: torch.nn.GRUCell's).  Reads what the training forward saved; the outputs are what the
 * weight-gradient GEMMs over all frames read.  Supported (ag_gfront_bwd_persist_ok): (S, fs) as for ag_gfront_persist_ok
 * and a grid of ceil(B/32) * (S/16 + ceil(fs/16)) workgroups <= n_cu (154 at B = 64, S = 1024, fs = 200); `ws`: the sticky
 * word + 8 KiB header (see ag_lstm_seq_fwd_persist).  Tensors fp32 and dense as above (G = 4 / 3); dgs, dxt and `ws` are
 * 16-byte aligned; a field the cell does not use must be NULL. */
typedef struct ag_front_bwd_args {
  int64_t struct_bytes; /* sizeof(ag_front_bwd_args) */
  int32_t cell;         /* 0 LSTM, 1 GRU */
  int32_t pad_;
  const float* ga;      /* both: [T,B,G*S] activated gates */
  const float* state;   /* LSTM: c_all [T+1,B,S]; GRU: hs [T+1,B,S] (hs[t] = h_{t-1}, hs[0] = 0) */
  const float* gh;      /* GRU: [T,B,3S], n slot = W_hn h_{t-1} + b_hn */
  const float* x;       /* both: [B,T*fs] the front's output, row pitch ldx */
  const float* dh_ext;  /* both, optional (NULL = zero): [T,B,S] = dL/dh_t, the stop head's; read only */
  const float* dx_ext;  /* both, optional (NULL = zero): [B,T*fs] = dL/dx_t, the conv trunk's, row pitch lddx (it may be
                           channel 0 of the trunk's gradient slab); read only */
  const float* w_hh;    /* both: [G*S,S] */
  const float* w_x;     /* both: W_ih[:, :fs], row pitch ldwx */
  const float* w_p;     /* both: [fs,S] */
  float* dgs;           /* both: [T,B,G*S] out.  LSTM: d gate pre-activations; GRU: dgi, d of the input-side pre-activations */
  float* dgh;           /* GRU: [T,B,3S] out, hidden side (the n slot times r) */
  float* dxt;           /* both: [T,B,fs] out, d pre-tanh of the projection */
  void* ws;
  int64_t ldx, lddx, ws_bytes;
  int32_t ldwx, T, B, S, fs, n_cu;
} ag_front_bwd_args;
int ag_gfront_bwd_persist_ok(int B, int S, int fs, int n_cu);
int ag_gfront_bwd(const ag_front_bwd_args* a, void* stream);

/* The BACKWARD through time of a STACKED front (2 <= nl <= 8 LSTMCell layers, L = nl - 1 the top one) in one persistent
 * launch (csrc/front_stack.hip).  Per frame t = T-1 .. 0, every term of frame T being zero:
 *   gx_t     = (dx_ext[t] + dg_{0,t+1} W_x)(1 - x_t^2)                     -> dxt[t]
 *   dh_{L,t} = dh_ext[t] + dg_{L,t+1} W_hh_L + gx_t W_p                    (the stop head's gradient lands on the top layer only)
 *   dh_{l,t} = dg_{l,t+1} W_hh_l + dg_{l+1,t} W_ih_{l+1}                   l < L
 *   dg_{l,t} = LSTM cell backward(dh_{l,t}, dc_{l,t+1})                    -> dgs[l][t]
 * Reads what ag_gfront_stack_fwd (or the per-frame forward) saved; the outputs are what the weight-gradient GEMMs over all
 * frames read.  fp32 MFMA; in bf16 mode (ag_set_precision) both operands of all four products are rounded in registers.
 * Supported (ag_gfront_stack_bwd_ok): 2 <= nl <= 8 (0 for nl = 1, which stays on ag_gfront_bwd); (S, fs) as for
 * ag_gfront_persist_ok; B >= 1 and a grid of ceil(B/32) * (nl * S/16 + ceil(fs/16)) workgroups <= min(n_cu, 256) (141 at the
 * reference's nl 2, B 32, S 1024, fs 200).  `ws` = ag_gfront_stack_bwd_ws_bytes() bytes: the sticky word + 8 KiB header
 * (dgs / dxt are the exchange buffers).
 *
 * Every tensor is fp32 and dense in the stated shape unless a pitch (in elements) is named; every dgs[l], dxt and `ws` are
 * 16-byte aligned.  The per-layer tables hold 8 entries: every entry below nl must be set, entries from nl on must be
 * NULL.  All of that, a wrong struct_bytes, T <= 0 and a pitch smaller than a row are refused with AG_ERR_ARG before any HIP
 * call; a shape outside the rule with AG_ERR_UNSUPPORTED. */
typedef struct ag_front_stack_bwd_args {
  int64_t struct_bytes; /* sizeof(ag_front_stack_bwd_args) */
  int32_t nl;           /* layers */
  int32_t pad_;
  const float* ga[8];   /* [T,B,4S] each: the activated gates (i, f, g, o) of layer l */
  const float* cs[8];   /* [T+1,B,S] each: cs[l][t] = c_{l,t-1}, cs[l][0] = 0 */
  const float* w_hh[8]; /* [4S,S] each */
  const float* w_in[8]; /* [0]: W_ih_0[:, :fs], [4S,fs] with row pitch ldwx; [l >= 1]: W_ih_l [4S,S] */
  float* dgs[8];        /* [T,B,4S] each, out: d gate pre-activations of layer l */
  const float* w_p;     /* [fs,S] */
  const float* x;       /* [B,T*fs] the front's output (after tanh), row pitch ldx */
  const float* dh_ext;  /* optional (NULL = zero): [T,B,S] = dL/dh_{L,t}, the stop head's; read only */
  const float* dx_ext;  /* optional (NULL = zero): [B,T*fs] = dL/dx_t, the conv trunk's, row pitch lddx; read only */
  float* dxt;           /* [T,B,fs] out, d pre-tanh of the projection */
  void* ws;
  int64_t ldx, lddx, ws_bytes;
  int32_t ldwx, T, B, S, fs, n_cu;
} ag_front_stack_bwd_args;
int ag_gfront_stack_bwd_ok(int B, int S, int fs, int nl, int n_cu);
int64_t ag_gfront_stack_bwd_ws_bytes(int B, int S, int fs, int nl);
int ag_gfront_stack_bwd(const ag_front_stack_bwd_args* a, void* stream);

/* One fused backward step of the Generator front (audiogan.py:428-460: LSTMCell -> tanh(Linear) fed back), frame t:
 *   gx     = dxa * (1 - x_t^2)                        d(pre-tanh) of the projection, stored to gx_out [B,Kp]
 *   dh     = dh_acc + gx * w_proj                      w_proj [Kp = frame size, H]; dh_acc [B,H] rows, pitch lddh
 *   (dgates, dc_prev) = LSTMCell backward(dh, dc_next; gates, c_prev, c_new)
 * ONE launch instead of tanh-backward + product + cell-backward.  dxa / x / gx_out are [B,Kp] row views (pitches in
 * floats, multiples of 4, 16-byte aligned); Kp % 16 == 0, H % 16 == 0; dc_next may be NULL (last frame). */
int ag_lstm_front_bwd_step(const float* dxa, int lddxa, const float* x, int ldx, float* gx_out, int ldgx, int Kp,
                           const float* w_proj, const float* dh_acc, int lddh, const float* gates, const float* c_prev,
                           const float* c_new, const float* dc_next, float* dgates, float* dc_prev, int B, int H,
                           void* stream);

/* ---------------------------------------------------------------------------
 * Masked BCE-with-logits per sample (audiogan.py:187-197 + :204-211 + the
 * "/ nframes ... .mean()" at :739-740,766,780,864,897), fused:
 *   l[b,t]  = x - x*target + m + log(exp(-m) + exp(-x-m)),  m = max(-x, 0)
 *   per[b]  = sum_{t < n[b]} l[b,t]               n = nframes_i64 (NULL: all T)
 *   loss   += scale * sum_b per[b] / n[b]         (scale = 1/B gives the mean)
 * bwd: dx[b,t] = gscale * scale / n[b] * (sigmoid(x) - target) * (t < n[b])
 * ------------------------------------------------------------------------- */
int ag_bce_logits_fwd(const float* x, int ldx, float target, const int64_t* nframes_i64,
                      float* per_sample, float* loss, float scale, int B, int T, void* stream);
int ag_bce_logits_bwd(const float* x, int ldx, float target, const int64_t* nframes_i64,
                      const float* gscale_dev, float scale, float* dx, int lddx, int B, int T,
                      void* stream);

/* The same loss on logits of any (row, column) pitch (element strides sxb, sxt), an optional target per row (target_rows,
 * NULL = `target` for every row) and loss[0] WRITTEN (= scale * sum_b per[b] / n[b]) by one launch; per_sample may be NULL.
 * The critic iteration scores real and fake clips in one pass (audiogan.py:739-740 + :766 + :780: targets 0.9 and 0). */
int ag_bce_logits_fwd_strided(const float* x, int64_t sxb, int64_t sxt, float target, const float* target_rows,
                              const int64_t* nframes_i64, float* per_sample, float* loss, float scale, int B, int T,
                              void* stream);
int ag_bce_logits_bwd_strided(const float* x, int64_t sxb, int64_t sxt, float target, const float* target_rows,
                              const int64_t* nframes_i64, const float* gscale_dev, float scale, float* dx, int64_t sdb,
                              int64_t sdt, int B, int T, void* stream);

/* ---------------------------------------------------------------------------
 * Elementwise helpers
 * ------------------------------------------------------------------------- */
/* y = act(x) on n contiguous floats (in place allowed) */
int ag_act_fwd(const float* x, float* y, int64_t n, int act, float slope, void* stream);
/* dx = dy * act'(.) using the saved OUTPUT y */
int ag_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int act, float slope,
               void* stream);
/* same on row-strided 2-D views [rows, cols] (frame slices of the generator's [B, T*frame] output) */
int ag_act_bwd2d(const float* dy, int lddy, const float* y, int ldy, float* dx, int lddx, int rows,
                 int cols, int act, float slope, void* stream);
/* y = a*x + b*y  on n contiguous floats */
int ag_axpby(const float* x, float* y, int64_t n, float a, float b, void* stream);

/* Feature-matching statistics over time of one activation h [B,C,L] (calc_dists, audiogan.py:341-350):
 *   m[b,c] = sum_t h / len[b];  cen_t = h_t - m * [t < len[b]];
 *   s[b,c] = sqrt(sum_t cen^2) / len[b];  f[b,c] = (sum_t cen^4)^(1/4) / len[b]
 * (sums over ALL t: the critic has zeroed padded steps).  bwd: dh from the gradients of m, s, f (any may be NULL). */
int ag_time_moments_fwd(const float* h, int64_t bs, int64_t cs, const int64_t* lens_i64, float* m, float* s, float* f,
                        int B, int C, int L, void* stream);
int ag_time_moments_bwd(const float* h, int64_t bs, int64_t cs, const int64_t* lens_i64, const float* gm,
                        const float* gs, const float* gf, float* dh, int64_t dbs, int64_t dcs, int B, int C, int L,
                        void* stream);

/* ---------------------------------------------------------------------------
 * Fused optimiser: check_grad + per-PARAMETER clip + update for a whole network
 * in two launches (audiogan.py:232-253, 693-694, 786-788, 909-921).
 *   pass 1: norm[i] = ||grad_i||_2 ; flags |= NaN / |g|>1e5
 *   pass 2: g = grad * min(1, clip/norm[i]) (clip == 0: no clip), then
 *     RMSprop (torch defaults): sq = a*sq + (1-a) g^2 ; p -= lr * g / (sqrt(sq)+eps)
 *     Adam (TF/torch defaults): m,v moments with bias correction from `step`
 * `norm_sum` receives sum_i norm[i] (the value clip_grad returns, :253).
 * ------------------------------------------------------------------------- */
typedef struct ag_opt_desc {
  float* p;
  const float* grad;
  float* s1; /* RMSprop: square_avg ; Adam: exp_avg    */
  float* s2; /* Adam: exp_avg_sq (unused for RMSprop)  */
  int64_t n;
} ag_opt_desc;

#define AG_OPT_RMSPROP 0
#define AG_OPT_ADAM 1
#define AG_FLAG_NAN 1
#define AG_FLAG_BIG 2

/* step_dev (optional): device-side optimiser step counter, incremented by ag_grad_norms and
 * read by ag_opt_step for Adam's bias correction, so a captured hipGraph of the train step
 * advances it on every replay.  When NULL the host value `step` is used.
 * ag_grad_norms needs a bound workspace of 2 * n * 256 floats (ag_bind_workspace): per-chunk sums of squares and flag
 * words, every slot written by its workgroup (nothing is zeroed in front of the launch, `flags` is WRITTEN).  finish = 1:
 * a second, one-workgroup launch turns the partials into norms / norm_sum / flags.  finish = 0 (round 4): that launch is
 * left out and the caller hands the same workspace to ag_opt_step as `part`: every workgroup of the update then sums its
 * tensor's 256 partials itself (same order, same value) and workgroup (0,0) writes norms_out / norm_sum / flags - two
 * launches per network and step instead of three plus two memset nodes.  part = NULL: `norms` as computed before. */
int ag_grad_norms(const ag_opt_desc* descs_dev, int n, float* norms, float* norm_sum,
                  int32_t* flags, float grad_scale, int32_t* step_dev, int finish, void* stream);
int ag_opt_step(const ag_opt_desc* descs_dev, int n, const float* norms, int kind, float lr,
                float clip, float grad_scale, float alpha_or_beta1, float beta2, float eps, int step,
                const int32_t* step_dev, const float* part, float* norms_out, float* norm_sum, int32_t* flags,
                void* stream);

/* ---------------------------------------------------------------------------
 * Exponential moving average of a parameter list (beyond the reference, like Adam): one launch for the whole list.
 *   per element, fp32:  e = fmaf(1 - d, p - e, e)      (the lerp form: exact when p == e; 1 - d == 1 stores p itself)
 *   d = decay                                 when warmup == 0
 *   d = min(decay, (1 + k) / (10 + k))        otherwise, in fp32, the same value in every workgroup;
 *       k = max(0, step_dev[0] - step0) with the optimiser's device step counter (read only: ag_grad_norms incremented
 *       it in an EARLIER launch on the same stream, so every workgroup reads one value), or the host value `k` when
 *       step_dev is NULL - as ag_opt_step does with `step`.  A captured launch therefore warms up on every replay.
 * `p` and the counter are never written; no workspace, no atomics, no host sync.
 * Grid: one workgroup per chunk of ag_ema_chunk() consecutive elements of one tensor.  map_dev is the chunk-to-tensor
 * map, [nchunks][2] int32 = (tensor index, chunk index inside that tensor), tensor i contributing
 * ceil(n_i / ag_ema_chunk()) entries; the caller builds it once and keeps it in device memory with the descriptors.
 * A tensor whose two pointers are equally aligned modulo 16 bytes moves in 16-byte accesses between a scalar head and
 * tail; any other tensor moves element by element.  Pointers are 4-byte aligned, every n >= 1, 0 <= decay <= 1.
 * ------------------------------------------------------------------------- */
typedef struct ag_ema_desc {
  float* ema;
  const float* p;
  int64_t n;
} ag_ema_desc;

int ag_ema_chunk(void);
int ag_ema_update(const ag_ema_desc* descs_dev, int n, const int32_t* map_dev, int nchunks, float decay, int warmup,
                  const int32_t* step_dev, int step0, int k, void* stream);

/* ---------------------------------------------------------------------------
 * Per-iteration summaries (audiogan.py:776-809, :875-884, :911-920: the scalars the reference logs) computed on the
 * device and gathered into a ring the host reads whenever it wants (audiogan_amd/summary.py).  Every reduction sums in
 * a fixed order (no float atomics): two runs give the same bits.
 *   ag_logit_summary   one critic output x [B,T] of any (row, column) pitch in elements (sxb, sxt):
 *                      out5 = { mean, std, hits, mask_sum, hits / mask_sum }; mean / std over ALL B*T entries, population
 *                      (ddof 0, what numpy's .mean() / .std() give; masked-out positions count), two-pass; hits = the
 *                      number of entries with t < nframes[b] and x > 0 (positive != 0) or x < 0 (positive == 0),
 *                      mask_sum = sum_b min(nframes[b], T).  One workgroup; B*T <= 2^22.
 *   ag_sqnorm_rows     part[b] = scale * sum_l gx[b,l]^2 / nframes[b] for gx [B,L] of row pitch ld (elements), one
 *                      workgroup per row; out (optional, NULL: the caller sums `part` itself, e.g. ag_summary_commit):
 *                      out[0] = (sum_b part[b], b ascending) / B, by a finishing launch.
 *   ag_vec_stats       out2 = { sign * mean(v), population std(v) } of v [n] contiguous, two-pass, one workgroup.
 *   ag_summary_commit  one row of the ring: column c < 16 = the 32-bit word at src[c] (float or int32 bits, copied as they
 *                      are) or imm[c] when src[c] is NULL; column 1 = the sequence number cursor[1]; column part_col (if
 *                      part != NULL) = (sum_b part[b], b ascending) / npart as ag_sqnorm_rows' finishing launch computes
 *                      it.  The row goes to ring[cursor[0]] (16 words per row); then cursor[0] = (cursor[0] + 1) %
 *                      capacity and cursor[1] += 1.  `desc_dev` is a DEVICE copy of the descriptor.
 * ------------------------------------------------------------------------- */
#define AG_SUMMARY_COLS 16
typedef struct ag_summary_desc {
  const void* src[AG_SUMMARY_COLS];
  uint32_t imm[AG_SUMMARY_COLS];
  const float* part;
  uint32_t* ring;    /* [capacity, 16] */
  int32_t* cursor;   /* [2]: next row, next sequence number */
  int32_t npart;
  int32_t part_col;
  int32_t capacity;
  int32_t pad_;
} ag_summary_desc;

int ag_logit_summary(const float* x, int64_t sxb, int64_t sxt, const int64_t* nframes_i64, int positive, float* out5, int B,
                     int T, void* stream);
int ag_sqnorm_rows(const float* gx, int64_t ld, const int64_t* nframes_i64, float scale, float* part, float* out, int B, int L,
                   void* stream);
int ag_vec_stats(const float* v, float sign, float* out2, int n, void* stream);
int ag_summary_commit(const ag_summary_desc* desc_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Held-out evaluation (audiogan_amd/evaluate.py; beyond the reference, which never scores its validation data): the
 * long-term average spectrum of ragged clips and the running statistics of a critic output.  Fixed-order sums, no atomics:
 * two runs give the same bits.
 *   ag_ltas_power    x [B, L] fp32 of row pitch ldx (elements), unit column stride; n_b = clamp(lens[b], 0, L) (lens NULL:
 *                    L).  Frames of 256 samples, hop 128, periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / 256): with
 *                    n_b >= 256 the frames j = 0 .. (n_b - 256) / 128, each wholly inside the clip (a tail shorter than
 *                    a hop is not covered); otherwise ONE frame, the clip followed by zeros.
 *                    out[b, k], k = 0..128 ([B, 129] contiguous) = mean over the clip's frames of |X_j[k]|^2, X_j the
 *                    256-point DFT of the windowed frame - the power itself, no logarithm; nframes_out[b] (int32, may be
 *                    NULL) = the frame count.  x[b, t] is never read for t >= n_b: padding may hold anything.  Window and
 *                    twiddles are cospif values of exact arguments; fp32 sums.  A clip of more than 16 frames is spread
 *                    over workgroups whose partial sums go to a bound workspace of ag_ltas_ws_numel(B, L) floats
 *                    (ag_bind_workspace; 0: none needed) and are added in ascending frame order by a second launch.
 *   ag_score_accum   x [B, T] logits of any (row, column) pitch in elements (sxb, sxt); n_b = clamp(nframes[b], 0, T)
 *                    (NULL: T).  ADDS to acc, six doubles the caller zeroes once per evaluation:
 *                      acc[0] += the number of clips with n_b >= 1
 *                      acc[1] += sum_b (sum_{t < n_b} bce(x[b,t], target)) / n_b    (audiogan.py:191-192, per element in fp32)
 *                      acc[2] += sum_b n_b
 *                      acc[3] += the valid entries with x > 0 (positive != 0) or x < 0 (positive == 0)
 *                      acc[4] += sum of x, acc[5] += sum of x^2, over the valid entries
 *                    so loss = acc[1] / acc[0], accuracy = acc[3] / acc[2], mean = acc[4] / acc[2] and
 *                    std = sqrt(max(0, acc[5] / acc[2] - mean^2)).  UNLIKE ag_logit_summary, whose mean / std run over all
 *                    B*T entries as the reference's numpy calls do, these run over the VALID entries only; masked
 *                    entries are never read.  One workgroup, every sum in double, one lane updates acc with plain loads
 *                    and stores; B*T <= 2^22.
 * ------------------------------------------------------------------------- */
int64_t ag_ltas_ws_numel(int B, int L);
int ag_ltas_power(const float* x, int64_t ldx, const int64_t* lens_i64, float* out, int32_t* nframes_out, int B, int L,
                  void* stream);
int ag_score_accum(const float* x, int64_t sxb, int64_t sxt, const int64_t* nframes_i64, float target, int positive,
                   double* acc, int B, int T, void* stream);

/* ---------------------------------------------------------------------------
 * Aligned distance of the held-out evaluation (evaluate.Evaluator(aligned=True), evaluate.aligned_distance): per-frame mel
 * cepstra and the dynamic-time-warping total between two cepstral sequences (csrc/evalalign.hip).  Both kernels are fp32
 * whatever ag_set_precision says, add in a fixed order and use no atomics: two runs give the same bits.  Both launchers
 * refuse bad arguments before their first HIP call.
 *   ag_melcep_frames x, ldx, lens, n_b and the framing exactly as ag_ltas_power: 256-sample periodic-Hann frames at hop 128,
 *                    j = 0 .. (n_b - 256) / 128 when n_b >= 256, otherwise ONE zero-padded frame; x[b, t] is never read
 *                    for t >= n_b.  F = the frame count of a clip of L samples is the frame capacity of the outputs.
 *                    Per frame j < nframes[b]:
 *                      P[k]  = |X_j[k]|^2, k = 0..128             -> power[b, j, k] ([B, F, 129] contiguous; NULL: not written)
 *                      E[m]  = sum_k mel[m, k] P[k], m = 0..23     (mel [24, 129] fp32 on the device, weights >= 0)
 *                      c[q]  = sum_m dct[q, m] logf(E[m] + 1e-10f), q = 0..12   (dct [13, 24] fp32 on the device)
 *                    -> cep[b, j, 0..12] = c, cep[b, j, 13..15] = 0 ([B, F, 16] contiguous).  nframes_out[b] (int32, may be
 *                    NULL) = the frame count.  Rows j >= nframes[b] of cep and power are never written.  fp32 sums in
 *                    ascending index order (a zero mel weight is skipped: it adds nothing).  The transform of a tile of 32
 *                    frames is an fp32 MFMA product (v_mfma_f32_32x32x2_f32: exact fp32 fma chains) of the windowed,
 *                    folded frames with twiddles that are cospif values of exact arguments; one launch, no workspace, and
 *                    a frame's bits do not depend on the tile it falls in.
 *   ag_dtw_cost      cep_a [B, Fa, 16], cep_b [B, Fb, 16] fp32 contiguous; n = clamp(nf_a[b], 1, Fa), m = clamp(nf_b[b], 1,
 *                    Fb) (int32; NULL: the capacity).  Rows at or past the counts and columns 0 and 13..15 are never read.
 *                      d(i, j) = sqrtf(sum_{q = 1..12} (a[i, q] - b[j, q])^2)      (fp32, sqrtf correctly rounded)
 *                      D(0, 0) = 2 d(0, 0)
 *                      D(i, j) = min(D(i-1, j) + d, D(i, j-1) + d, D(i-1, j-1) + 2 d) over the predecessors that exist
 *                    out[b] = D(n-1, m-1), the raw total of the symmetric step pattern: every path has weight n + m, so the
 *                    caller divides by n + m.  ag_dtw_cost(a, b) and ag_dtw_cost(b, a) give the same bits.
 *                    Fa, Fb <= 1024 (clips of up to 131200 samples); one workgroup per pair, one thread per row of a.
 * ------------------------------------------------------------------------- */
int ag_melcep_frames(const float* x, int64_t ldx, const int64_t* lens_i64, const float* mel, const float* dct, float* cep,
                     int32_t* nframes_out, float* power, int B, int L, void* stream);
int ag_dtw_cost(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b, float* out, int B, int Fa,
                int Fb, void* stream);

/* ---------------------------------------------------------------------------
 * ag_dtw_pairs (csrc/evalpairs.hip): the total of ag_dtw_cost for P pairs drawn from two BANKS of sequences, without
 * gathered copies (evaluate.Evaluator(crossed=True, draws=k), evaluate.aligned_distance_matrix).
 *   cep_a [Na, Fa, 16], cep_b [Nb, Fb, 16] fp32 contiguous rows of ag_melcep_frames; nf_a [Na], nf_b [Nb] int32 counts
 *   (NULL: the capacity).  ia, ib: int32 [P] on the device, both given or both NULL.
 *     lists     out[p] = the DTW total of a[clamp(ia[p], 0, Na-1)] against b[clamp(ib[p], 0, Nb-1)] - the kernel clamps: a
 *               wrong index is a wrong pair, never an address outside the banks
 *     NULL      the cross product: P = Na Nb and out[i Nb + j] is pair (i, j)
 *   under exactly the contract of ag_dtw_cost (the same recursion, counts clamped to [1, capacity], columns 1..12 only, rows
 *   at or past the counts never read), and with THE BITS ag_dtw_cost returns for the same two sequences.
 *   Two forms, chosen on the host from the capacities alone:
 *     wave form       min(Fa, Fb) <= 64 and max(Fa, Fb) <= 256: one wave per pair, four pairs per 256-thread workgroup, the
 *                     longer side in the wave's own slice of dynamic LDS (4 * F * 48 bytes <= 48 KB), no barrier in the
 *                     step loop; the side of at most 64 frames supplies the rows (the sides are exchanged when that is b;
 *                     the output layout does not change)                                     "dtw_pairs_wave_kernel"
 *     workgroup form  otherwise: the scheme of ag_dtw_cost with pair indices and Fb * 48 bytes of dynamic LDS
 *                                                                                            "dtw_pairs_wg_kernel"
 *   No atomics, no spin, no dependency between workgroups, trip counts n + m - 1 <= 2047: two runs give the same bits.
 *   Refused from host code before any HIP call (AG_ERR_ARG): null cep_a, cep_b or out; exactly one of ia / ib; P <= 0 or
 *   P > 2^24; NULL lists with P != Na Nb; Na or Nb outside 1..65535; Fa or Fb outside 1..1024.
 * ------------------------------------------------------------------------- */
int ag_dtw_pairs(const float* cep_a, const int32_t* nf_a, int Na, int Fa, const float* cep_b, const int32_t* nf_b, int Nb,
                 int Fb, const int32_t* ia, const int32_t* ib, float* out, int P, void* stream);

/* ---------------------------------------------------------------------------
 * ag_dtw_align (csrc/dtwalign.hip): the recursion of ag_dtw_cost WITH ITS PATH, for cutting a transcribed utterance into
 * words against a reference sequence of word templates (audiogan_amd/align.py, ingest --utterances).
 *   cep_a [B, Fa, 16] (the utterance: rows), cep_b [B, Fb, 16] (the reference: columns), nf_a, nf_b exactly as ag_dtw_cost
 *   takes them: counts clamped to [1, capacity] (NULL: the capacity), columns 1..12 only, rows at or past the counts never
 *   read, Fa, Fb <= 1024, one workgroup per pair and one thread per row of a.
 *   total[b]   = D(n-1, m-1) with THE BITS ag_dtw_cost returns for the same pair (the same fmaf chain, sqrtf, fminf order
 *                and d + d on the diagonal).
 *   The path   from (n-1, m-1) back to (0, 0); at every cell it goes to the predecessor whose candidate value
 *                D(i-1, j-1) + 2 d,  D(i-1, j) + d,  D(i, j-1) + d
 *              equals the minimum in fp32, and among several that do to THE FIRST IN THAT ORDER: the diagonal, then
 *              (i-1, j), then (i, j-1).  On row 0 it goes left, in column 0 up.
 *   lo[b, j], hi[b, j]  (int32 [B, Fb]) = the first and the last row of a on the path in column j, for j < m.  lo[0] = 0,
 *              hi[m-1] = n-1, lo[j] <= hi[j], lo[j+1] is hi[j] or hi[j] + 1.  Columns j >= m are never written.
 *   ws, ws_bytes  the decisions, two bits per cell: ag_dtw_align_ws(Fa, Fb) = Fa * ceil(Fb / 16) * 4 bytes PER PAIR (at most
 *              256 KB; 0 for capacities outside 1..1024), B of them, 4-byte aligned, supplied by the caller - the launcher
 *              allocates nothing and there is no bound slot.  Each thread packs 16 consecutive columns of its row into one
 *              word and stores it when it is full or the row ends; the walk back (thread 0, after the forward loop's last
 *              barrier and one more) reads them, at most n + m - 2 moves, and never follows a code out of the matrix.
 *              What the workspace holds afterwards is not part of the contract.
 *   No atomics, no spin, no dependency between workgroups; trip counts are uniform across the workgroup and at most 2047:
 *   two runs give the same bits.                                                                  "dtw_align_kernel"
 *   Refused from host code before any HIP call (AG_ERR_ARG): null cep_a, cep_b, total, lo, hi or ws; B <= 0; Fa or Fb outside
 *   1..1024; ws_bytes < B * ag_dtw_align_ws(Fa, Fb).
 *   ag_dtw_align_forward: the same launch without the walk back (lo, hi not written) - for tools/prof_dtwalign.py, which
 *   times it to split the cost; nothing in the package calls it.
 * ------------------------------------------------------------------------- */
int64_t ag_dtw_align_ws(int Fa, int Fb);
int ag_dtw_align(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b, float* total, int32_t* lo,
                 int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb, void* stream);
int ag_dtw_align_forward(const float* cep_a, const int32_t* nf_a, const float* cep_b, const int32_t* nf_b, float* total,
                         int32_t* lo, int32_t* hi, void* ws, int64_t ws_bytes, int B, int Fa, int Fb, void* stream);

/* ---------------------------------------------------------------------------
 * Pitch measures of the held-out evaluation (evaluate.Evaluator(aligned=True, pitch=True), evaluate.pitch_distance;
 * csrc/pitch.hip): per-frame pitch candidates from the normalised cross-correlation, and the sums of F0 and voicing
 * differences along the path of ag_dtw_align.  Both kernels are fp32 whatever ag_set_precision says, use no atomics, no spin
 * and no dependency between workgroups, and add in a fixed order: two runs give the same bits.  Both launchers refuse bad
 * arguments from host code before their first HIP call (AG_ERR_ARG).
 *   ag_pitch_frames  x, ldx, lens, n_b and the framing exactly as ag_melcep_frames: frame j starts at sample 128 j, there are
 *                    (n_b - 256) / 128 + 1 of them when n_b >= 256 and otherwise ONE; x[b, t] is never read for t >= n_b;
 *                    F = the frame count of a clip of L samples is the capacity of the outputs; rows j >= nframes[b] are
 *                    never written.  So frame j here is frame j of the cepstra and the path of ag_dtw_align indexes both.
 *                    Constants: W = ag_pitch_window() = 256, TMIN = ag_pitch_tmin() = 20, TMAX = ag_pitch_tmax() = 127 (at
 *                    8 kHz: 400 Hz down to 63 Hz); lags 19..128 are computed, 110 values.  Per frame:
 *                      s[t]    = x[b, 128 j + t], t = 0..383; 0 (and not read) at and past n_b.  center != 0: the mean of
 *                                the segment's valid samples (fp32, a fixed order of the kernel's own that depends on the
 *                                segment alone) is subtracted from the valid samples; the zeros stay zero
 *                      r(tau)  = sum_{t < 256} s[t] s[t + tau],  e(tau) = sum_{t < 256} s[t + tau]^2,  e0 = e(0): each sum
 *                                ONE fmaf chain in ascending t
 *                      phi(tau) = den > 0 ? r(tau) / sqrtf(den) : 0,  den = e0 * e(tau)  (sqrtf and the division correctly
 *                                rounded)
 *                      M       = max of phi over tau = 20..127
 *                      tau*    = the SMALLEST tau in 20..127 with phi(tau) >= phi(tau - 1), phi(tau) >= phi(tau + 1) and
 *                                phi(tau) >= octf * M (the product rounded once); 0 when M <= 0 or none qualifies - the
 *                                first strong peak, which is what avoids octave errors
 *                    -> lag[b, j] = tau* (int32 [B, F]); peak[b, j, 0..3] = phi(tau* - 1), phi(tau*), phi(tau* + 1), e0 / 256
 *                    (fp32 [B, F, 4]; zeros and e0 / 256 when tau* = 0); nccf[b, j, 0..109] = phi(19..128), columns 110 and
 *                    111 zero (fp32 [B, F, ag_pitch_nccf_width() = 112], NULL: not written); nframes_out[b] (int32, may be
 *                    NULL).  The logarithm and the sub-sample refinement are the caller's, in float64
 *                    (evaluate.pitch_cents).  One workgroup per (clip, tile of ag_pitch_tile() = 8 frames), one wave per
 *                    frame, two lags a lane; a frame's bits do not depend on the tile it falls in.  The tile's samples are
 *                    staged with 16-byte loads when x is 16-byte aligned and ldx is a multiple of 4
 *                    ("pitch_frames_kernel<1>"), one float at a time otherwise ("pitch_frames_kernel<0>"): same bits.
 *                    Refused: null x, lag or peak; B <= 0; L <= 0; ldx < L; octf outside (0, 1]; more than 65535 tiles a
 *                    clip (L of 67 108 096 samples or more).
 *   ag_pitch_path_accum  pc_a [B, Fa] (the rows of the alignment: the fake), pc_b [B, Fb] (the columns: the real clip):
 *                    fp32 cents, NEGATIVE = unvoiced.  lo, hi int32 [B, Fb] as ag_dtw_align leaves them; m = clamp(nf_b[b],
 *                    1, Fb) (NULL: Fb).  The path's cells are, for each column j < m, the rows lo[j]..hi[j], each cell once;
 *                    row indices are clamped into [0, Fa - 1], so a wrong index is a wrong cell, never an address outside.
 *                    Columns j >= m of lo, hi and pc_b are never read.  out[b, 0..4] (fp32 [B, ag_pitch_path_words() = 5],
 *                    plain stores): the cells; the cells with both frames voiced; the cells whose voicing differs; the
 *                    both-voiced cells with |a - b| > gross (cents); sum (a - b)^2 over the both-voiced cells.  The counts
 *                    are integers until the store (exact: a path has at most 2047 cells).  The sum is one fmaf chain per
 *                    column over ascending rows, then a fixed-order combination of the columns.  One workgroup of 256
 *                    threads per pair.                                                   "pitch_path_accum_kernel"
 *                    Refused: null pc_a, pc_b, lo, hi or out; B <= 0; Fa or Fb outside 1..1024.
 * ------------------------------------------------------------------------- */
int ag_pitch_window(void);
int ag_pitch_tmin(void);
int ag_pitch_tmax(void);
int ag_pitch_nccf_width(void);
int ag_pitch_tile(void);
int ag_pitch_path_words(void);
int ag_pitch_frames(const float* x, int64_t ldx, const int64_t* lens_i64, float octf, int center, int32_t* lag, float* peak,
                    float* nccf, int32_t* nframes_out, int B, int L, void* stream);
int ag_pitch_path_accum(const float* pc_a, const float* pc_b, const int32_t* lo, const int32_t* hi, const int32_t* nf_b,
                        float gross, float* out, int B, int Fa, int Fb, void* stream);

/* ---------------------------------------------------------------------------
 * ag_resample_poly (csrc/resample.hip): polyphase windowed-sinc resampling of ragged rows of PCM frames to the models'
 * rate (audio.resample, ingest.build_store).  Replaces librosa.load(wav, sr=8000) of the reference's preprocessing
 * (preprocess.py:24, preprocess-fisher.py:232).  fp32 whatever ag_set_precision says; no atomics, no workspace, one launch.
 *   src        B rows of interleaved frames, src_pitch ELEMENTS apart; src_kind 0 = fp32, 1 = int16; channels 1..8.
 *              Row b holds frames in_start .. in_start + len_b - 1 of its signal (absolute frame indices),
 *              len_b = clamp(src_len[b], 0, n_in) (int64 on the device; NULL: n_in).  Every other frame reads as zero and
 *              is never loaded.  The mono sample of a frame is (x_0 + .. + x_{C-1}) * (1.0f / C), channels added in order
 *              in fp32; int16 values are then scaled by 2^-15.
 *   bank       [L, taps] fp32 contiguous on the device (audio.resample_bank), half = (taps - 1) / 2.
 *   dst[b, n]  n < n_out, rows dst_pitch floats apart, = y[out_start + n] with
 *                y[N] = sum_{t = 0}^{taps - 1} bank[p, t] x[base - half + t],  base = (N M) div L,  p = (N M) mod L,
 *              N M in 64 bits.  Each output is one fmaf chain over t ascending from a zero accumulator, whatever n, b,
 *              out_start or the tile it falls in: a signal resampled in chunks (a row holding the frames its outputs need
 *              plus half frames either side, with the two starts set) has the bits of the same signal resampled at once.
 *              ALL n_out entries of every row are written; the caller slices at ceil(len_b L / M).
 *   One workgroup per (row, tile of up to 1024 outputs): the tile's input window is converted and downmixed once into
 *   LDS, the bank sits beside it at its own odd row pitch.                                        "resample_poly_kernel"
 *   ag_resample_ok: 1 when L, M >= 1, taps is odd and >= 3, L * taps * 4 <= 65536, channels are 1..8 and kind is 0 or 1.
 *   Refused from host code before any HIP call (AG_ERR_ARG): anything the predicate refuses; a negative size, start or B;
 *   a null src, dst or bank with work to do; src_pitch < n_in * channels; dst_pitch < n_out; M above 2^20; out_start
 *   or n_out past 2^40; more than 2^31 - 1 tiles in one launch.  B = 0 or n_out = 0: AG_OK with no launch.
 * ------------------------------------------------------------------------- */
int ag_resample_ok(int L, int M, int taps, int channels, int src_kind);
int ag_resample_poly(const void* src, int src_kind, int channels, long long src_pitch, const long long* src_len,
                     long long n_in, long long in_start, const float* bank, int L, int M, int taps, float* dst,
                     long long dst_pitch, long long n_out, long long out_start, int B, void* stream);

/* ---------------------------------------------------------------------------
 * ag_clip_facts, ag_clip_gather (csrc/clipstore.hip): the loader's minibatch assembled on the device from a packed store of
 * every clip (dataset.DeviceWordStore, dataset.ClipBatch).  They stand where the reference's pick_word scans, normalises
 * and stacks float64 rows on the host at every draw (dataset.py:48-77).  fp32 whatever ag_set_precision says; no atomics,
 * no workspace, one launch each.
 *   The packed store (laid out by the Python side, relied on here): clip c is bank[start[c] : start[c] + cap[c]] (fp32);
 *   start int64 - the bank may exceed 2^31 floats - and every start[c] a multiple of 4 floats; cap int32.  bank is 16-byte
 *   aligned, its allocation a multiple of 4 floats, so a 16-byte load at t % 4 == 0, t < cap[c] never leaves it.
 *   ag_clip_facts   per clip c < n_clips: n_out[c] (int32) = the index after the last sample whose bits are not those of
 *                   +0.0 or -0.0 (a denormal and a NaN are not zero), 0 if there is none - the loader's length rule
 *                   (dataset.py:52); peak_out[c] = max |x| over the clip, +inf for an infinite sample and a NaN if any
 *                   sample is one (formed as the largest |x| bit pattern, so no flushed or dropped value takes part).
 *                   Both are order-independent: exact.  One workgroup per clip.                        "clip_facts_kernel"
 *   ag_clip_gather  for b < B, t < L_out, c = ids[b] (int64 on the device, 0 <= c < n_clips: the CALLER's duty):
 *                     out[b * ld_out + t] = t < min(n[c], L_out) ? bank[start[c] + t] / peak[c] : 0
 *                   the division correctly rounded in fp32 (= the host's float64 divide followed by the float32 cast);
 *                     len_out[b] (int64, may be NULL) = frame > 0 ? roundup(n[c], frame) : n[c], not cropped to L_out.
 *                   Nothing outside [0, L_out) of a row is written.  Grid (ceil(L_out / 1024), B), four consecutive
 *                   samples per thread with 16-byte loads and stores when out is 16-byte aligned and ld_out % 4 == 0
 *                   (the last, partial group of a row with scalar stores), one sample per access otherwise.
 *                                                                       "clip_gather_kernel<1>" (16-byte) / "<0>" (scalar)
 *   Refused from host code before any HIP call (AG_ERR_ARG): a negative n_clips, B, L_out or frame; B above 65535; a null
 *   or misaligned bank, a null start, cap, n, peak, ids or out with work to do; ld_out < L_out.  n_clips = 0, or B = 0:
 *   AG_OK with no launch.
 * ------------------------------------------------------------------------- */
int ag_clip_facts(const float* bank, const long long* start, const int32_t* cap, int32_t* n_out, float* peak_out,
                  long long n_clips, void* stream);
int ag_clip_gather(const float* bank, const long long* start, const int32_t* n, const float* peak, const long long* ids,
                   int B, float* out, long long ld_out, int L_out, long long* len_out, int frame, void* stream);

/* ---------------------------------------------------------------------------
 * ag_join_facts, ag_join_clips (csrc/join.hip): generated words put next to each other on the device (synth.Voice.say_batch).
 * The rows are ragged clips whose lengths are on the device; both launches read them there, so a sentence is joined with no
 * host read.  The reference has no inference path (audiogan.py trains and logs).  fp32 whatever ag_set_precision says; no
 * atomics, no workspace, one launch each.
 *   The window of row r < R: wave[r * ld + off' .. + n'), off' = clamp(off[r], 0, L_in), n' = clamp(n[r], 0, L_in - off')
 *   (off, n int32 on the device; off is arbitrary, so samples are loaded 4 bytes at a time).
 *   ag_join_facts   per row: the peak = the largest |x| bit pattern of the window (as ag_clip_facts forms it);
 *                     bad_out[r] (int32) = 1 when that pattern is >= +inf's - the window holds a NaN or an infinity - and
 *                     gain_out[r] = 0 then; else gain_out[r] = peak > 0 ? target / peak (correctly rounded) : 1.
 *                     target <= 0: every gain is 1 (bad is still formed).  n' = 0: peak 0.  Order-free: exact.
 *                   One workgroup per row.                                                              "join_facts_kernel"
 *   ag_join_clips   sentence s < S owns segments k = sent_ptr[s] .. sent_ptr[s + 1] - 1 (int32 [S + 1], ascending, within
 *                   0 .. K; at most ag_join_max_segments() = 1024 of them); segment k is the window of row seg_row[k] (int32
 *                   [K]; a row may serve any number of segments).  THE PLAN of a sentence, in integers, n_k its windows' n':
 *                     f_k = min(F, n_k / 2)                                   the fade length of segment k
 *                     join[k] >= 0: a pause of min(join[k], pause_max) zero samples between k and k + 1
 *                     join[k] <  0: an overlap ov_k = min(-join[k], n_k / 2, n_{k+1} / 2)          (integer divisions)
 *                     st_0 = 0,  st_{k+1} = st_k + n_k + pause  or  st_k + n_k - ov_k;  the sentence's last join is ignored
 *                     total = st_last + n_last (0 for an empty sentence);  out_len[s] (int64) = total, NOT cropped to O_cap.
 *                   With these clamps at most two segments cover a sample: k* = the last k with st_k <= t, and k* - 1.
 *                   Sample i of segment k, j = n_k - 1 - i, weighs w = ramp[(i F) / f_k] if i < f_k, ramp[(j F) / f_k] if
 *                   j < f_k, else 1 (the two regions cannot meet), with the coefficient c = fmul(gain[row], w).  For t < O_cap:
 *                     two covering segments a < b:  out[s * ld_out + t] = fadd(fmul(x_a, c_a), fmul(x_b, c_b))
 *                     one:                          fmul(x, c)
 *                     none (a pause, t >= total):   0
 *                   each operation rounded once to fp32 - never a contracted fma.  EVERY t < O_cap of every sentence is
 *                   written.  ramp: fp32 [F] on the device (kernels.join_ramp: sin^2(pi (i + 0.5) / (2 F)), float64 rounded
 *                   once), not read when F = 0.  Grid (ceil(O_cap / 1024), S); every workgroup forms its sentence's plan in
 *                   LDS (one exclusive scan of 1024 advances), then each thread takes four consecutive samples: one binary
 *                   search, one 16-byte store when out is 16-byte aligned and ld_out % 4 == 0, four 4-byte stores
 *                   otherwise - the same bits.                          "join_clips_kernel<1>" (16-byte) / "<0>" (scalar)
 *                   What the tables hold cannot send a load outside wave: a seg_row outside 0 .. R - 1 is an empty segment,
 *                   sent_ptr is clamped to 0 .. K, segments past a sentence's 1024th are dropped.
 *   Refused from host code before any HIP call (AG_ERR_ARG): a negative R, L_in, K, O_cap or pause_max; S outside 0 .. 65535;
 *   F outside 0 .. 4096; K > 1024 S (some sentence holds more than ag_join_max_segments(); a sentence's own count is on the
 *   device: the CALLER's duty, synth.Voice checks it on the host); min(K, 1024) (L_in + pause_max) > 2^31 - 1 (a sentence
 *   could pass the int32 plan); ld < L_in; ld_out < O_cap; a null pointer with work to do; a NaN target.  R = 0 (facts) or
 *   S = 0 (clips): AG_OK with no launch.
 * ------------------------------------------------------------------------- */
int ag_join_max_segments(void);
int ag_join_facts(const float* wave, long long ld, int L_in, const int32_t* off, const int32_t* n, int R, float target,
                  float* gain_out, int32_t* bad_out, void* stream);
int ag_join_clips(const float* wave, long long ld, int L_in, const int32_t* off, const int32_t* n, const float* gain, int R,
                  const int32_t* seg_row, const int32_t* join, const int32_t* sent_ptr, int K, int S, int pause_max,
                  const float* ramp, int F, float* out, long long ld_out, int O_cap, long long* out_len, void* stream);

/* ---------------------------------------------------------------------------
 * ag_frame_power, ag_activity_segments (csrc/activity.hip): short-time energy activity detection on the resampled rows
 * (audio.activity, ingest.build_store(trim / split)).  They stand where the reference's preprocessing cuts words by a forced
 * alignment (preprocess-fisher.py:145-146) or keeps windows by an amplitude threshold (preprocess.py:25-27).  fp32 whatever
 * ag_set_precision says; no atomics, no workspace, one launch each.
 *   ag_frame_power
 *     src        B rows of fp32 samples, src_pitch ELEMENTS apart, 4-byte aligned.  Row b holds samples in_start .. in_start +
 *                len_b - 1 of its signal (absolute sample indices), len_b = clamp(src_len[b], 0, n_in) (int64 on the device;
 *                NULL: n_in).  Every other sample reads as zero and is never loaded.
 *     dst[b, j]  j < n_frames, rows dst_pitch floats apart, = the power of frame f = f_start + j: the sum of x^2 over samples
 *                f hop .. f hop + win - 1 times fp32(1 / win), f hop in 64 bits.  ALL n_frames entries of every row are written.
 *     THE ORDER  with g = gcd(win, hop), hq = hop / g, wq = win / g the signal falls into blocks of g samples that start at
 *                multiples of g of the absolute sample index;
 *                  S_k = the fmaf chain s = fmaf(x, x, s) over samples k g .. k g + g - 1 ascending, from s = 0;
 *                  P_f = ((0 + S_{f hq}) + S_{f hq + 1}) + .. + S_{f hq + wq - 1};   dst = P_f * (1.0f / win).
 *                That is the whole of a frame's arithmetic, whatever b, j, the tile, in_start or f_start: a signal processed
 *                in chunks (a row holding just the samples its frames read, with the two starts set) has the bits of the
 *                same signal processed at once.
 *     One workgroup per (row, tile of ag_frame_power_tile(win, hop) <= 256 frames): the tile's samples are staged once into
 *     LDS (16-byte loads at aligned addresses, whatever the row's own alignment) at an odd block pitch, thread k forms block
 *     sum k, thread j frame j.                                                                       "frame_power_kernel"
 *     ag_frame_power_ok: 1 when 1 <= hop <= win <= 4096.  ag_frame_power_tile: the launch's tile of frames (0 when refused).
 *     Refused from host code before any HIP call (AG_ERR_ARG): anything the predicate refuses; a negative size, start or B;
 *     a null dst, or a null src with n_in > 0, with work to do; src not 4-byte aligned; src_pitch < n_in; dst_pitch <
 *     n_frames; f_start or n_frames past 2^40; more than 2^31 - 1 tiles in one launch.  B = 0 or n_frames = 0: AG_OK, no launch.
 *   ag_activity_segments
 *     power [B, F] fp32, rows power_pitch floats apart; nf[b] (int32, clamped to 0 .. F) frames of row b; len[b] (int64,
 *     clamped at 0) its samples; seg [B, K, 2] int64; count [B] int32; pmax [B] fp32.  Per row, in integers but for the two
 *     fp32 operations named:
 *       1. pmax = max_f power[f] (order-free: exact; -0 counts below +0);  thr = max(pmax * ratio, floor): one fp32 multiply,
 *          one max;  active[f] = power[f] > thr.
 *       2. close: an inactive run strictly between two active frames and shorter than min_gap frames becomes active.
 *       3. drop: after closing, an active run shorter than min_run frames becomes inactive.
 *       4. pad and merge: a run of frames [a, b) becomes samples [max(0, (a - pad) hop), min(len, (b - 1 + pad) hop + win));
 *          runs whose sample ranges overlap or touch become one.
 *       5. count[b] = the number of runs left, even above K; seg[b, k] = (start, end) for k < min(count, K), ascending;
 *          entries past that are NOT written.
 *       6. nf = 0 or no active frame: count = 0 (pmax = 0 for nf = 0).  A NaN or an infinity among the row's nf powers:
 *          count = -1, pmax = the quiet NaN 0x7fc00000, no segment.
 *     One workgroup per row, the frames in chunks of ag_activity_chunk() = 1024 whose flags are one ballot word per wave; the
 *     run state is carried in registers from chunk to chunk, so a row of any length needs 128 bytes of LDS.
 *                                                                                                 "activity_segments_kernel"
 *     Refused from host code before any HIP call (AG_ERR_ARG): a negative min_gap, min_run, pad, K or F; B outside 0 .. 65535;
 *     a win / hop pair ag_frame_power_ok refuses; with B > 0: power_pitch < F, a null nf, len, count or pmax, a null power
 *     with F > 0, a null seg with K > 0.  B = 0: AG_OK with no launch.
 * ------------------------------------------------------------------------- */
int ag_frame_power_ok(int win, int hop);
int ag_frame_power_tile(int win, int hop);
int ag_frame_power(const float* src, long long src_pitch, const long long* src_len, long long n_in, long long in_start, int win,
                   int hop, float* dst, long long dst_pitch, long long f_start, long long n_frames, int B, void* stream);
int ag_activity_chunk(void);
int ag_activity_segments(const float* power, long long power_pitch, const int32_t* nf, int F, const long long* len, float ratio,
                         float floor_, int min_gap, int min_run, int pad, int win, int hop, long long* seg, int K,
                         int32_t* count, float* pmax, int B, void* stream);

/* ---------------------------------------------------------------------------
 * ag_sheet_render (csrc/sheet.hip): a minibatch of ragged clips drawn as ONE contact sheet (audiogan_amd/sheet.py: render,
 * SheetWriter) - per clip a waveform envelope over a spectrogram.  It stands where the reference plots every sample's waveform
 * on the host (audiogan.py:639-653, :674, :930).  The clips' lengths stay on the device and nothing is read back.  fp32
 * whatever ag_set_precision says; no atomics, no workspace, one launch; two runs give the same bytes.
 *   wave [B, L] fp32, rows ld floats apart; n_b = clamp(lens[b], 0, L) (int64 on the device; NULL: L).  wave[b, t] is never
 *   read for t >= n_b.  power [B, F, 129] fp32 contiguous and nframes [B] int32 as ag_melcep_frames leaves them;
 *   nf_b = clamp(nframes[b], 0, min(F, Wt)); power[b, j, :] is never read for j >= nf_b.  thresholds fp32 [256], ascending
 *   (sheet.thresholds); cmap uint8 [256, 3] (R, G, B).  bg, paper, ink: colours as 0x00BBGGRR.
 *   THE GRID  Wt = ceil(L / 128) pixel columns per tile - one per hop of 128 samples - and Ht = Hw + 129 rows; tile b sits at
 *     grid cell (b div cols, b mod cols), its top left pixel at
 *       y0 = gutter + (b div cols) (Ht + gutter),   x0 = gutter + (b mod cols) (Wt + gutter)
 *     and the image img, uint8 [H, W, 3] contiguous at ANY byte alignment, must be exactly
 *       H = gutter + rows (Ht + gutter),   W = gutter + cols (Wt + gutter),   rows cols >= B.
 *     Every pixel outside a tile - gutters, grid cells b >= B - is bg.
 *   THE ENVELOPE, rows 0 .. Hw - 1 of a tile.  peak_b = max |wave[b, t]| over t < n_b, from 0, a NaN dropped (fmaxf: the order
 *     does not matter).  Column j < ceil(n_b / 128) covers the samples t = 128 j .. 128 j + 127 with t < n_b; vmax and vmin are
 *     their fmaxf / fminf (both 0 if every one is a NaN).  A value lands on the row
 *       row(v) = (int) rintf(fminf(fmaxf(fmul(fsub(1.0f, fdiv(v, peak_b)), half), 0.0f), top)),
 *       half = 0.5f * (float)(Hw - 1),   top = (float)(Hw - 1)
 *     each operation rounded once to fp32 (fdiv correctly rounded, as in ag_clip_gather; never a contracted fma), rintf to the
 *     nearest even: +peak is row 0, -peak row Hw - 1.  Rows min(row(vmax), row(vmin)) .. max(..) are ink, the others paper.
 *     peak_b = 0: the one row (Hw - 1) div 2 is ink in every such column.  Columns j >= ceil(n_b / 128) are bg.
 *   THE SPECTROGRAM, rows Hw .. Hw + 128 of a tile; row Hw + s shows bin k = 128 - s: bin 0 is at the bottom.
 *     Pmax_b = the fmaxf of power[b, j, k] over j < nf_b, all k, from 0 (order-free: exact).  For j < nf_b and
 *     P = power[b, j, k] the level is the largest l with P >= fmul(thresholds[l], Pmax_b); 0 if there is none (so for a NaN
 *     P) or if Pmax_b is 0.  The pixel is cmap[level].  No logarithm is taken: the host folds it into the table,
 *     thresholds[l] = fp32(10^((l / 255 - 1) range_db / 10)), and the search (8 steps over the table in LDS) is exact where
 *     a logf would differ between devices and libraries.  Columns j >= nf_b are bg.
 *   One workgroup per (grid cell, tile of ag_sheet_tile_columns() = 32 columns); its prologue redoes the clip's two maxima,
 *   stages the tile's frames of power in LDS as they lie in memory and reads them back across the frames at the odd pitch
 *   129, and forms the envelope rows of its columns one wave per column.  The workgroups' rectangles - a tile's columns with
 *   the gutter below, the gutter to the right behind a tile's last column, the sheet's top / left gutter with the first row /
 *   column of cells - tile the image: EVERY pixel is written exactly once.  A chunk of 32 pixel rows is formed in LDS at the byte
 *   phase its row has in memory and stored as whole dwords; single bytes only at a row segment's ragged ends.
 *                                                                                                    "sheet_render_kernel"
 *   Refused from host code before any HIP call (AG_ERR_ARG): a null wave, power, nframes, thresholds, cmap or img; B, F or
 *   L <= 0; L above 2^30; ld < L; Hw outside 3 .. 4096; gutter outside 0 .. 16; cols <= 0; an H x W that is not the grid's
 *   exactly; more than 65535 grid cells.
 * ------------------------------------------------------------------------- */
int ag_sheet_tile_columns(void);
int ag_sheet_render(const float* wave, long long ld, const long long* lens, int L, const float* power, const int32_t* nframes,
                    int F, int B, const float* thresholds, const unsigned char* cmap, unsigned bg, unsigned paper, unsigned ink,
                    int cols, int Hw, int gutter, unsigned char* img, int H, int W, void* stream);

/* ---- Conv2DLSTMCell (reference cells.py:4-103: convolutional LSTM with peepholes and TF layer normalisation) ----------
 * Pointwise / normalisation pieces (csrc/convlstm.hip); the convolution runs on ag_conv1d_engine, one launch per kernel row.
 * Every map is [H, B, C, W] contiguous (rows x batch = the 1-D engine's batch axis, W = its time axis); peephole weights
 * [H, F, W]; gate blocks of the convolution output y [H,B,4F,W] along C in TF.split order j | i | f | o (cells.py:66).
 *   peephole_fwd  j, i_pre = i + W_ci c, f_pre = f + W_cf c, o_raw  (cells.py:66-70; w_ci / w_cf may be NULL: no peepholes)
 *   cell_fwd      c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j);  o_pre = o_raw + W_co c'   (:77-82)
 *   out_fwd       h = sigmoid(o) tanh(c)                                                               (:88-89)
 *   layer_norm    tf.contrib.layers.layer_norm: per sample over (H, W, F), gamma / beta per feature, eps inside the sqrt
 * The backward forms take the forward's inputs again (nothing is saved besides mean / rstd); dc of peephole_bwd is
 * ACCUMULATED into (it also receives the cell path's dc); weight gradients are written (summed over the batch in a fixed
 * order); layer_norm_bwd writes per-sample partials [B,F] of dgamma / dbeta for a fixed-order column sum by the caller. */
int ag_convlstm_peephole_fwd(const float* y, const float* c, const float* w_ci, const float* w_cf, float* j, float* i_pre,
                             float* f_pre, float* o_raw, int H, int B, int F, int W, void* stream);
int ag_convlstm_peephole_bwd(const float* dj, const float* di, const float* df, const float* d_o, const float* c,
                             const float* w_ci, const float* w_cf, float* dy, float* dc, float* dw_ci, float* dw_cf, int H,
                             int B, int F, int W, void* stream);
int ag_convlstm_cell_fwd(const float* j, const float* i_, const float* f_, const float* c, const float* o_raw,
                         const float* w_co, float forget_bias, float* c_new, float* o_pre, int H, int B, int F, int W,
                         void* stream);
int ag_convlstm_cell_bwd(const float* j, const float* i_, const float* f_, const float* c, const float* c_new,
                         const float* w_co, float forget_bias, float* dc_new, const float* do_pre, float* dj, float* di,
                         float* df, float* dc, float* dw_co, int H, int B, int F, int W, void* stream);
int ag_convlstm_out_fwd(const float* o, const float* c, float* h, int64_t n, void* stream);
int ag_convlstm_out_bwd(const float* o, const float* c, const float* dh, float* d_o, float* dc, int64_t n, void* stream);
int ag_layer_norm_hbfw_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* mean, float* rstd,
                           int H, int B, int F, int W, void* stream);
int ag_layer_norm_hbfw_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                           float* dgamma_part, float* dbeta_part, int H, int B, int F, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOGAN_HIP_H */

"""Recurrent blocks of the hot path.

  LSTMSeqFn     NN.LSTM layer over a padded batch      audiogan.py:498-503, :543, :214-229, :315
  GFrontFn      LSTMCell stack + tanh(proj) feedback   audiogan.py:377-386, :409-410, :428-460
  front_sample  the same frame loop for sampling       audiogan.py:444-460 (stop draws, early exit), :922-935

The per-time-step work is a product with only B (clips per GPU) rows.  When shapes allow
(B <= 64, sizes multiples of 8, 16-byte aligned rows -- true for every BASELINE config) the
steps run on the fused / skinny kernels of lstm_step.hip, a whole NN.LSTM layer being enqueued
by ONE C call; other shapes take the generic GEMM + pointwise path.  Everything that does not
depend on the recurrence (input projections, weight gradients, stopper head) is batched over
all time steps into a few large GEMMs.
"""
import contextlib

import torch

from . import kernels as K
from .kernels import ACT_NONE, ACT_TANH
from .common import Bf16Images, WNGroup, _zeros_like_list, grad_target


# set inside losses.only_stopper_trains: the backward that runs there is the REINFORCE update of the stop head, whose
# gradient is wanted in the stopper's parameters ONLY (audiogan.py:897-903) - not in the block's input either
STOPPER_ONLY = [False]


def _prod(*a, **k):
    from .ops import _prod as f
    return f(*a, **k)


def _small(A, B, Cm, tb=False, beta=0.0, bias=None, act=ACT_NONE, res=None):
    """Cm = act(A @ op(B) + beta*Cm + bias + res) for a product with few rows"""
    if res is None and K.skinny_ok(A, B, tb):
        K.skinny_gemm(A, B, Cm, tb=tb, beta=beta, bias=bias, act=act)
    else:
        K.gemm(A, B, Cm, tb=tb, beta=beta, bias=bias, res=res, act=act)


def _linear1(x, w, b, y):
    """y [M,1] = x @ w^T + b for a Linear with ONE output (the stop head): one wave per row (ag_rowdot_fwd) instead of a
    64-wide MFMA tile that is 98 % padding plus a split-K second stage"""
    if K.rowdot_ok(x, w):
        K.rowdot_fwd(x, w, b, y)
    else:
        K.gemm(x, w, y, tb=True, bias=b)


def _bcast_rows(v, rows):
    """[n] -> a [rows, n] view whose rows are all `v` (row pitch 0): a second bias for K.gemm's `res`"""
    return v.view(1, -1).expand(rows, v.numel())


def _small_acc(A, B, Cm, tb=False):
    """Cm += A @ op(B)"""
    if K.skinny_ok(A, B, tb):
        K.skinny_gemm(A, B, Cm, tb=tb, atomic=True)
    else:
        K.gemm(A, B, Cm, tb=tb, beta=1.0)


# --------------------------------------------------------------------------------------
# LSTM layer over a padded sequence (uni- or bidirectional), NN.LSTM parameter layout
# --------------------------------------------------------------------------------------
def _wih16(w, ndir, Fx):
    """[ndir * 4H, Fx] bfloat16: the x-columns of every direction's W_ih stacked - the B operand of the input projections
    (per direction: a row block, k contiguous) and of the input gradient dx = [dg_0 | dg_1] @ stack (k strided).  ``w``: the
    layer's PARAMETERS (forward and backward alike - a saved ``.data`` alias has neither their version nor their epoch); the
    images belong to the first of them (common.Bf16Images)"""
    H4 = w[0].size(0)
    im = getattr(w[0], '_ag_wih16', None)
    if im is None or im.stack.shape != (ndir * H4, Fx) or im.stack.device != w[0].device:
        im = w[0]._ag_wih16 = Bf16Images(ndir * H4, Fx, w[0].device)
    for d in range(ndir):
        im.fill(d * H4, w[4 * d], Fx)
    return im.stack


class LSTMSeqFn(torch.autograd.Function):
    """x: [T,B,Fx]; lengths: int64 [B] on device or None; ``static``: None or [B,Fc], a time-invariant part
    of the input (the layer sees cat([x_t, static]) at every step, audiogan.py:541); weights per direction:
    (w_ih [4H,Fx+Fc], w_hh [4H,H], b_ih [4H], b_hh [4H]).  Returns y [T,B,D*H] with zeros at padded steps
    (pad_packed_sequence semantics, audiogan.py:214-229).

    The static part is projected ONCE per clip (c @ W_ih[:, Fx:]^T + biases -> [B,4H]) and added inside the
    step kernel, instead of being concatenated to all T frames and multiplied T times; its weight / input
    gradients come from the time sum of dgates (the same pass that gives the bias gradient).

    bf16 storage (x arrives as bfloat16): x, the layer output y, dgates' operand copy and dx are bfloat16 in HBM and every
    large product runs on ag_gemm_h (ops._prod picks the kernel by its operands' dtype); gate pre-activations, cell states
    and the persistent kernels' exchange stay fp32.  Storage decides the W_ih operand (the bf16 stack / the fp32 weight),
    the dgates operand (one [T,B,ndir*4H] bf16 tensor the persistent launch writes beside its fp32 exchange buffer / that
    buffer itself) and the form of dx (one product over both directions / one per direction); the rest is common."""

    @staticmethod
    def forward(ctx, x, lengths, ndir, static, *w):
        T, B, Fx = x.shape
        H = w[1].size(1)
        dev = x.device
        x2 = x.contiguous().view(T * B, Fx)
        Fc = static.size(1) if static is not None else 0
        assert w[0].size(1) == Fx + Fc
        st = static.contiguous() if static is not None else None
        s16 = x.dtype == torch.bfloat16
        if s16:     # (the persistent launches write y / read dy as bf16)
            assert K.lstm_step_ok(B, H) and K.lstm_persist_ok(B, H, ndir, dev) and K.lstm_persist_bwd_ok(B, H, ndir, dev), \
                'bf16 storage needs the persistent LSTM launches (modules.Discriminator.classify checks this)'
            wst = _wih16(w, ndir, Fx)
        y = torch.empty(T, B, ndir * H, device=dev, dtype=torch.bfloat16 if s16 else torch.float32)
        gates_all, c_all, whh, cbs = [], [], [], []
        fused = K.lstm_step_ok(B, H)
        for d in range(ndir):
            w_ih, w_hh, b_ih, b_hh = w[4 * d:4 * d + 4]
            g = torch.empty(T, B, 4 * H, device=dev)
            g2 = g.view(T * B, 4 * H)
            wx = wst[d * 4 * H:(d + 1) * 4 * H] if s16 else w_ih.data[:, :Fx]
            # b_ih + b_hh: one rides as the GEMM's bias, the other as a `res` whose row pitch is 0 (the same row for every
            # output row) - no launch to add the two vectors first
            if st is not None:
                cb = torch.empty(B, 4 * H, device=dev)
                K.gemm(st, w_ih.data[:, Fx:], cb, tb=True, bias=b_ih.data, res=_bcast_rows(b_hh.data, B))
                if fused:
                    _prod(x2, wx, g2, tb=True)
                    cbs.append(cb)
                else:       # generic per-step path: fold the static term into the pre-activations up front
                    g.copy_(cb.unsqueeze(0).expand(T, B, 4 * H))
                    _prod(x2, wx, g2, tb=True, beta=1.0)
            else:
                _prod(x2, wx, g2, tb=True, bias=b_ih.data, res=_bcast_rows(b_hh.data, T * B))
            c = torch.empty(T + 1, B, H, device=dev)   # c[k+1] = cell after the k-th processed step
            if not (fused and K.lstm_persist_ok(B, H, ndir, dev)):
                c[0].zero_()                           # (the persistent launch writes c_0 = 0 itself)
            gates_all.append(g)
            c_all.append(c)
            whh.append(w_hh.data.contiguous())
        hbuf = [torch.empty(2, B, H, device=dev) for _ in range(ndir)]
        if fused:
            K.lstm_seq_fwd(gates_all, whh, c_all, hbuf, y, lengths, static=cbs if cbs else None)
        else:
            for d in range(ndir):
                g, c = gates_all[d], c_all[d]
                hbuf[d][0].zero_()
                for k in range(T):
                    t = k if d == 0 else T - 1 - k
                    hp, hn = hbuf[d][k & 1], hbuf[d][(k + 1) & 1]
                    if k > 0:
                        K.gemm(hp, whh[d], g[t], tb=True, beta=1.0)
                    K.lstm_cell_fwd(g[t], c[k], c[k + 1], h_out=hn, y_out=y[t, :, d * H:(d + 1) * H],
                                    h_prev=hp, valid=lengths, t=t)
        ctx.ndir, ctx.has_len, ctx.has_static = ndir, lengths is not None, st is not None
        ctx.params = w
        ctx.save_for_backward(x2, y, lengths if lengths is not None else x2.new_empty(0),
                              st if st is not None else x2.new_empty(0),
                              *(gates_all + c_all + [t_.data for t_ in w]))
        ctx.shape = (T, B, Fx, H)
        return y

    @staticmethod
    def backward(ctx, dy):
        T, B, Fx, H = ctx.shape
        ndir, H4 = ctx.ndir, 4 * H
        sv = ctx.saved_tensors
        x2, y2 = sv[0], sv[1].view(T * B, ndir * H)
        lengths = sv[2] if ctx.has_len else None
        st = sv[3] if ctx.has_static else None
        gates_all, c_all, w = list(sv[4:4 + ndir]), list(sv[4 + ndir:4 + 2 * ndir]), sv[4 + 2 * ndir:]
        dev = x2.device
        s16 = x2.dtype == torch.bfloat16
        dy = dy.contiguous()
        whh = [w[4 * d + 1].contiguous() for d in range(ndir)]
        dgs = [torch.empty(T, B, H4, device=dev) for _ in range(ndir)]
        # (the persistent launch - all there is on bf16 storage - keeps dh / dc in its own exchange buffers)
        dhb = None if s16 else [torch.empty(2, B, H, device=dev) for _ in range(ndir)]
        dcb = None if s16 else [torch.empty(2, B, H, device=dev) for _ in range(ndir)]
        dg16 = torch.empty(T, B, ndir * H4, device=dev, dtype=torch.bfloat16) if s16 else None
        wg = any(ctx.needs_input_grad[4:])
        need_ds = st is not None and ctx.needs_input_grad[3]
        # sum over time of dgates (the static input and the biases see every step's gradient): the persistent launch sums it
        # in the registers of the threads that produce dgates; other paths leave it to a pass over dgates below
        want_sum = st is not None and (wg or need_ds)
        dgsums = [torch.empty(B, H4, device=dev) for _ in range(ndir)] if want_sum else None
        have_sum = False
        if s16 or (B <= 256 and H % 2 == 0):
            kw = dict(dg16=[dg16[:, :, d * H4:(d + 1) * H4] for d in range(ndir)]) if s16 else {}
            have_sum = K.lstm_seq_bwd(gates_all, whh, c_all, dy, dgs, dhb, dcb, lengths, dgsum=dgsums, **kw)
            assert have_sum or not (s16 and want_sum)
        else:
            for d in range(ndir):
                g, c, dg = gates_all[d], c_all[d], dgs[d]
                for k in reversed(range(T)):
                    t = k if d == 0 else T - 1 - k
                    dpass = dhb[d][(k + 1) & 1]
                    K.lstm_cell_bwd(g[t], c[k], c[k + 1], None if k == T - 1 else dhb[d][k & 1],
                                    dy[t, :, d * H:(d + 1) * H], None if k == T - 1 else dcb[d][(k + 1) & 1],
                                    dg[t], dcb[d][k & 1], dh_pass=dpass, valid=lengths, t=t)
                    if k > 0:
                        K.gemm(dg[t], whh[d], dpass, beta=1.0)
        # dgates of direction d as the gradient products read them: rows in (t, b) order, [T*B, 4H]
        dgo = [dg16.view(T * B, ndir * H4)[:, d * H4:(d + 1) * H4] if s16 else dgs[d].view(T * B, H4) for d in range(ndir)]
        dx2 = None
        if s16 and ctx.needs_input_grad[0]:
            dx2 = torch.empty(T * B, Fx, device=dev, dtype=torch.bfloat16)
            _prod(dg16.view(T * B, ndir * H4), _wih16(ctx.params, ndir, Fx), dx2)     # both directions in ONE product
        elif not s16:
            dx2 = torch.empty(T * B, Fx, device=dev)
        dstatic = torch.zeros_like(st) if need_ds else None
        for d in range(ndir):
            w_ih = w[4 * d]
            if not s16:
                K.gemm(dgo[d], w_ih[:, :Fx], dx2, beta=0.0 if d == 0 else 1.0)
            if want_sum and not have_sum:
                # (read right below and by the weight-gradient products: complete at once, also inside a deferral scope)
                K.col_sum(dgs[d].view(T, B * H4), dgsums[d].view(-1), accumulate=False, defer=False)
            if need_ds:
                K.gemm(dgsums[d], w_ih[:, Fx:], dstatic, beta=1.0)
        outs = [] if wg else [None] * (4 * ndir)
        # a parameter takes a gradient only if it required one when the FORWARD ran (needs_input_grad: a forward under
        # common.frozen leaves its .grad untouched whatever the flag says by now); a direction none of whose parameters
        # did is skipped
        needs = [[n_ and p_.requires_grad for n_, p_ in zip(ctx.needs_input_grad[4 + 4 * d:8 + 4 * d], ctx.params[4 * d:4 * d + 4])]
                 for d in range(ndir)]          # (... and still does now: a backward under a freeze)
        tgs = [[grad_target(p_) if n_ else None for p_, n_ in zip(ctx.params[4 * d:4 * d + 4], needs[d])]
               for d in range(ndir)] if wg else []
        # every parameter gradient goes straight into ``.grad``: nothing reads it before the optimiser, so the second
        # stages of the split-K products and column sums below may wait for the enclosing scope's ONE launch
        direct_all = wg and all(t_ is not None for tg, nd_ in zip(tgs, needs) if any(nd_) for t_ in tg)
        with (K.deferred_reduces() if direct_all else contextlib.nullcontext()):
            for d in range(ndir if wg else 0):
                if not any(needs[d]):
                    outs += [None, None, None, None]
                    continue
                w_ih, w_hh, tg = w[4 * d], w[4 * d + 1], tgs[d]
                direct = all(t_ is not None for t_ in tg)
                if direct:      # accumulate straight into .grad
                    dw_ih, dw_hh = tg[0], tg[1]
                else:
                    dw_ih, dw_hh = torch.zeros_like(w_ih), torch.zeros_like(w_hh)
                _prod(dgo[d], x2, dw_ih[:, :Fx] if st is not None else dw_ih, ta=True, beta=1.0, defer=direct_all)
                if st is not None:
                    K.gemm(dgsums[d], st, dw_ih[:, Fx:], ta=True, beta=1.0, defer=direct_all)
                if T > 1:
                    # h_prev of processing step k is the layer output of step k-1 (zero at padded steps, where dgates is
                    # zero as well): one time step earlier for the forward direction, one later for the reverse one
                    if d == 0:
                        _prod(dgo[d][B:], y2[:(T - 1) * B, :H], dw_hh, ta=True, beta=1.0, defer=direct_all)
                    else:
                        _prod(dgo[d][:(T - 1) * B], y2[B:, H:2 * H], dw_hh, ta=True, beta=1.0, defer=direct_all)
                # (the bias sums read fp32 dgates on either storage)
                src = dgsums[d] if want_sum else dgs[d].view(T * B, H4)
                if direct:
                    K.col_sum(src, tg[2])
                    K.col_sum(src, tg[3])
                    outs += [None, None, None, None]
                    continue
                db = torch.zeros(H4, device=dev)
                K.col_sum(src, db)
                outs += [dw_ih, dw_hh, db, db.clone()]
        dx = dx2.view(T, B, Fx) if (dx2 is not None and ctx.needs_input_grad[0]) else None
        return (dx, None, None, dstatic) + tuple(outs)


# --------------------------------------------------------------------------------------
# Generator recurrent front: T x [LSTMCell stack -> tanh(proj) fed back, stopper logit]
# --------------------------------------------------------------------------------------
def _frames_buffer(front, B, n, dev):
    """where the front writes its frames x [B, n].  When the block feeds a conv trunk that keeps its activations in one
    [B, ctot, n] slab (``front.slab_channels = ctot``, set by the Generator), x IS channel 0 of a fresh slab - the trunk
    finds its input in place (ops.GTrunkFn) instead of copying 2 MB per forward."""
    ctot = getattr(front, 'slab_channels', 0)
    # (device tensors only: the kernels write through raw pointers; under the CPU kernel model of the tests torch's version
    # counter of the shared storage would see the trunk's writes as in-place edits of the saved frames)
    if ctot and ctot > 1 and torch.device(dev).type == 'cuda':
        return torch.empty(B, ctot, n, device=dev)[:, 0, :]
    return torch.empty(B, n, device=dev)


def _front_pre(zc, wz, b_ih, b_hh, pre, gru):
    """the part of the fronts' gate pre-activations that does not wait for the frame loop, all frames in one GEMM, in the form
    the persistent launches take: pre [T,B,G*S] = zc_t @ W_ih[:, fs:]^T + b_ih + b_hh.  LSTM: the second bias as a `res` of row
    pitch 0 (no launch to add the two vectors first).  GRU: only the r / z halves of b_hh ride along, b_hn stays apart (it
    sits inside r * (...))"""
    T, B, Fz = zc.shape
    zc2, pre2 = zc.contiguous().view(T * B, Fz), pre.view(T * B, pre.size(2))
    if gru:
        S = b_hh.numel() // 3
        bias = b_ih.clone()
        bias[:2 * S] += b_hh[:2 * S]
        K.gemm(zc2, wz, pre2, tb=True, bias=bias)
    else:
        K.gemm(zc2, wz, pre2, tb=True, bias=b_ih, res=_bcast_rows(b_hh, T * B))


def _stop_head_grads(ds, h2, dws, i, **sum_kw):
    """the stop head's part of a front's backward, s_t = h_t W_s^T + b_s: returns ds [B,T] as rows in (t, b) order [T*B,1]
    and, when ``dws`` is given, leaves dW_s = ds^T h in dws[i] and db_s = sum ds in dws[i + 1] (``sum_kw``: col_sum's)"""
    ds_tb = ds.t().contiguous().view(-1, 1)
    if dws is not None:
        K.gemm(ds_tb, h2, dws[i], ta=True)
        K.col_sum(ds_tb, dws[i + 1], **sum_kw)
    return ds_tb


def _ext_grads(ds_tb, sw, dx, T, B, S):
    """the external gradients of a persistent front backward (ag_gfront_bwd), read where they are: dL/dh_t (the stop
    head's, if any) from a [T,B,S] product, dL/dx_t from the trunk's gradient (any row pitch: channel 0 of its slab) - no
    [T,B,S+fs] staging tensor to fill and copy into"""
    dh_ext = None
    if ds_tb is not None:
        dh_ext = torch.empty(T, B, S, device=ds_tb.device)
        K.gemm(ds_tb, sw, dh_ext.view(T * B, S))
    return dh_ext, dx if (dx is None or dx.stride(1) == 1) else dx.contiguous()


def _one_launch(ok, T, wx, *dims):
    """is a front's frame loop ONE persistent launch?  A frame to run, wx = W_ih[:, :fs] of unit stride along its rows, and
    the launch's predicate: ``ok`` is a K.*_ok, looked up on K by the caller at call time, ``dims`` its arguments"""
    return T > 0 and wx.stride(1) == 1 and ok(*dims)


def _xprev_rows(x, xt, T, B, fs):
    """x_{t-1} for t = 1..T-1 as rows in (t, b) order, the operand of the W_ih[:, :fs] gradient: the persistent forward left
    the frames time-major (xt); otherwise a transposed copy of x [B, T*fs]"""
    if xt is not None:
        return xt[:T - 1].view((T - 1) * B, fs)
    return x.view(B, T, fs)[:, :T - 1].transpose(0, 1).contiguous().view((T - 1) * B, fs)


class GFront(object):
    """WN items: per layer [w_ih, w_hh, b_ih, b_hh] * num_layers, then [proj.w, proj.b, stop.w, stop.b]"""

    def __init__(self, frame_size, num_layers, state_size):
        self.fs, self.nl, self.ss = frame_size, num_layers, state_size
        self.slab_channels = 0
        self.group = WNGroup()


class GFrontFn(torch.autograd.Function):
    """zc: [T,B,noise+embed] contiguous.  Returns x [B,T*fs], s [B,T].  Frame t's LSTM input is
    [x_{t-1}, zc_t] (audiogan.py:439); the zc part of every frame's gate product is done in one
    GEMM up front, only the fed-back x_{t-1} and h products stay in the sequential loop."""

    @staticmethod
    def forward(ctx, zc, front, *params):
        T, B, Fz = zc.shape
        fs, nl, S = front.fs, front.nl, front.ss
        dev = zc.device
        ctx.set_materialize_grads(False)
        prep = front.group.prepare()
        lw = [[p.w for p in prep[4 * l:4 * l + 4]] for l in range(nl)]
        pw, pb, sw, sb = [p.w for p in prep[4 * nl:4 * nl + 4]]
        x = _frames_buffer(front, B, T * fs, dev)
        gates = [torch.empty(T, B, 4 * S, device=dev) for _ in range(nl)]
        hs = [torch.empty(T, B, S, device=dev) for _ in range(nl)]
        cs = [torch.empty(T + 1, B, S, device=dev) for _ in range(nl)]
        wx, wz = lw[0][0][:, :fs], lw[0][0][:, fs:]
        _front_pre(zc, wz, lw[0][2], lw[0][3], gates[0], gru=False)
        xt = None
        if nl > 1 and _one_launch(K.gfront_stack_ok, T, wx, B, S, fs, nl, dev):
            # the whole frame loop of ALL layers (every LSTMCell step + projection, fed back) in ONE launch; it writes every
            # layer's history as the per-frame path does: the backward (one launch or the per-frame chain) reads either
            xt = torch.empty(T, B, fs, device=dev)
            K.gfront_stack_fwd_persist(gates, wx, [lw[l][0] for l in range(1, nl)], [lw[l][1] for l in range(nl)],
                                       [lw[l][2] + lw[l][3] for l in range(1, nl)], pw, pb, hs, cs, x, xt)
        elif nl == 1 and _one_launch(K.gfront_persist_ok, T, wx, B, S, fs, dev):
            # the whole frame loop (LSTMCell step + projection, fed back) in ONE launch, weights resident in registers; the
            # frames are also written time-major (xt): what the weight gradient of W_ih[:, :fs] reads in backward
            xt = torch.empty(T, B, fs, device=dev)
            K.gfront_fwd_persist(gates[0], wx, lw[0][1], pw, pb, hs[0], cs[0], x, xt)
        else:
            GFrontFn._fwd_frames(T, B, fs, S, nl, x, gates, hs, cs, lw, wx, pw, pb)
        s = torch.empty(T * B, 1, device=dev)
        _linear1(hs[-1].view(T * B, S), sw, sb, s)
        ctx.front, ctx.key = front, front.group._key[1:]
        ctx.dims = (T, B, Fz)
        ctx.has_xt = xt is not None
        ctx.save_for_backward(zc, x, *(gates + hs + cs + ([xt] if xt is not None else [])))
        return x, s.view(T, B).t()

    @staticmethod
    def _fwd_frames(T, B, fs, S, nl, x, gates, hs, cs, lw, wx, pw, pb):
        """per-frame chain, one launch per operation (any number of layers); gates[0] holds the z / c pre-activations"""
        fused = [K.lstm_step_ok(B, S, x[:, :fs], wx)] + [K.lstm_step_ok(B, S)] * (nl - 1)
        for l in range(nl):
            cs[l][0].zero_()                       # (the persistent launches write c_0 = 0 themselves)
        h0 = torch.zeros(B, S, device=x.device)
        bsum = [lw[l][2] + lw[l][3] for l in range(nl)]
        for t in range(T):
            xprev = x[:, (t - 1) * fs:t * fs] if t > 0 else x[:, :fs]
            for l in range(nl):         # layer 0 reads the fed-back frame, the others the layer below
                if l > 0:
                    _small(hs[l - 1][t], lw[l][0], gates[l][t], tb=True, bias=bsum[l])
                if fused[l]:
                    K.lstm_step_fwd(gates[l][t], xprev if l == 0 else None, wx if l == 0 else None,
                                    hs[l][t - 1] if t > 0 else h0, lw[l][1], cs[l][t], cs[l][t + 1], hs[l][t], first_step=t == 0)
                else:
                    if t > 0 and l == 0:
                        K.gemm(xprev, wx, gates[0][t], tb=True, beta=1.0)
                    if t > 0:
                        K.gemm(hs[l][t - 1], lw[l][1], gates[l][t], tb=True, beta=1.0)
                    K.lstm_cell_fwd(gates[l][t], cs[l][t], cs[l][t + 1], h_out=hs[l][t])
            _small(hs[-1][t], pw, x[:, t * fs:(t + 1) * fs], tb=True, bias=pb, act=ACT_TANH)

    @staticmethod
    def _bwd_frames(T, B, fs, S, nl, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws):
        """per-frame chain, one launch per operation (any number of layers)"""
        dev = x.device
        # dxa[:, frame t] accumulates dL/dx_t: output gradient + feedback from frame t+1
        dxa = dx.contiguous().clone() if dx is not None else torch.zeros(B, T * fs, device=dev)
        # dha[l][t] accumulates dL/dh_l[t]: recurrent term from frame t+1, the layer above / the
        # projection at frame t, and (top layer) the stopper head
        dha = [torch.zeros(T, B, S, device=dev) for _ in range(nl)]
        if ds is not None:
            ds_tb = _stop_head_grads(ds, hs[-1].view(T * B, S), dws, 4 * nl + 2)
            K.gemm(ds_tb, sw, dha[-1].view(T * B, S))
        dgs = [torch.empty(T, B, 4 * S, device=dev) for _ in range(nl)]
        dxt = torch.empty(T, B, fs, device=dev)      # d(pre-tanh) of the projection, per frame
        dcs = [[torch.zeros(B, S, device=dev), torch.empty(B, S, device=dev)] for _ in range(nl)]
        for t in reversed(range(T)):
            gx = dxt[t]
            K.act_bwd2d(dxa[:, t * fs:(t + 1) * fs], x[:, t * fs:(t + 1) * fs], gx, ACT_TANH)
            _small_acc(gx, pw, dha[-1][t])                                   # through the projection
            for l in reversed(range(nl)):
                K.lstm_cell_bwd(gates[l][t], cs[l][t], cs[l][t + 1], dha[l][t], None,
                                dcs[l][(t + 1) & 1] if t < T - 1 else None, dgs[l][t], dcs[l][t & 1])
                if t > 0:
                    _small_acc(dgs[l][t], lw[l][1], dha[l][t - 1])           # into h_l[t-1]
                if l > 0:
                    _small_acc(dgs[l][t], lw[l][0], dha[l - 1][t])           # into h_{l-1}[t]
                elif t > 0:
                    _small_acc(dgs[0][t], wx, dxa[:, (t - 1) * fs:t * fs])   # into x_{t-1}
        return dgs, dxt

    @staticmethod
    def _bwd_frames_fused(T, B, fs, S, x, dx, ds, gates, cs, w_hh, wx, pw, sw, hs, dws, nl, persist):
        """single-layer front: ONE persistent launch where the shape fits (``persist``: ag_gfront_bwd), else TWO launches
        per frame: dacc[t] = [dL/dh_t | dL/dx_t] lives in one [B, S+fs] row so that  dacc[t-1] += dgates_t @ [W_hh |
        W_ih[:, :fs]]  is ONE product, and the tanh backward of the projection, its product and the cell backward are one
        fused step (ag_lstm_front_bwd_step)."""
        dev = x.device
        ds_tb = _stop_head_grads(ds, hs.view(T * B, S), dws, 4 * nl + 2, defer=False) if ds is not None else None
        dgs = torch.empty(T, B, 4 * S, device=dev)
        dxt = torch.empty(T, B, fs, device=dev)
        if persist:
            # the whole loop in ONE launch, [W_hh | W_x] and W_p resident in registers (ag_gfront_bwd)
            dh_ext, dx_ext = _ext_grads(ds_tb, sw, dx, T, B, S)
            K.gfront_bwd_persist(gates, cs, x, dh_ext, dx_ext, w_hh, wx, pw, dgs, dxt)
            return [dgs], dxt
        dacc = torch.zeros(T, B, S + fs, device=dev)
        if dx is not None:
            dacc[:, :, S:].copy_(dx.view(B, T, fs).transpose(0, 1))
        if ds_tb is not None:
            K.gemm(ds_tb, sw, dacc.view(T * B, S + fs)[:, :S])
        wcat = torch.cat([w_hh, wx], 1)                # [4S, S+fs]
        dcs = [torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)]
        for t in reversed(range(T)):
            K.lstm_front_bwd_step(dacc[t, :, S:], x[:, t * fs:(t + 1) * fs], dxt[t], pw, dacc[t, :, :S], gates[t], cs[t],
                                  cs[t + 1], dcs[(t + 1) & 1] if t < T - 1 else None, dgs[t], dcs[t & 1])
            if t > 0:
                K.skinny_gemm(dgs[t], wcat, dacc[t - 1], atomic=True)
        return [dgs], dxt

    @staticmethod
    def backward(ctx, dx, ds):
        front = ctx.front
        fs, nl, S = front.fs, front.nl, front.ss
        T, B, Fz = ctx.dims
        prep = front.group.prepare()
        assert front.group._key[1:] == ctx.key, 'parameters changed between forward and backward'
        sv = ctx.saved_tensors
        zc, x = sv[0], sv[1]
        gates, hs, cs = sv[2:2 + nl], sv[2 + nl:2 + 2 * nl], sv[2 + 2 * nl:2 + 3 * nl]
        xt = sv[2 + 3 * nl] if ctx.has_xt else None
        dev = zc.device
        lw = [[p.w for p in prep[4 * l:4 * l + 4]] for l in range(nl)]
        pw, sw = prep[4 * nl].w, prep[4 * nl + 2].w
        wx = lw[0][0][:, :fs]
        # no parameter of the block needs a gradient (FGSM-style input-gradient passes): skip every weight-gradient
        # product and leave ``.grad`` untouched
        wg = any(ctx.needs_input_grad[2:])
        items = front.group.items
        if dx is None and ds is not None and (STOPPER_ONLY[0] or not ctx.needs_input_grad[0]) and \
                not any(it['v'].requires_grad or it['g'].requires_grad for it in items[:4 * nl + 2]):
            # REINFORCE backward of the stop head alone (audiogan.py:897-903: every other generator parameter is
            # frozen): s_t = h_t W_s^T + b_s, so only dW_s = ds^T h and db_s = sum ds are wanted - no frame loop
            dws = [None] * len(items)
            dws[4 * nl + 2], dws[4 * nl + 3] = _zeros_like_list([items[4 * nl + 2]['v'], items[4 * nl + 3]['v']])
            _stop_head_grads(ds, hs[-1].view(T * B, S), dws, 4 * nl + 2)
            return (None, None) + tuple(front.group.backward(dws, ctx.needs_input_grad[2:]))
        dws = front.group.zero_dws() if wg else None
        # (the persistent launch takes frame sizes the fused per-frame step does not: any multiple of 8 up to its panel width)
        persist = nl == 1 and _one_launch(K.gfront_bwd_persist_ok, T, wx, B, S, fs, dev)
        if persist or (nl == 1 and T > 0 and (S + fs) % 4 == 0 and K.lstm_front_bwd_ok(B, S, fs, x[:, :fs], x[:, :fs])
                       and K.skinny_ok(gates[0][0], lw[0][1], False)):
            dgs, dxt = GFrontFn._bwd_frames_fused(T, B, fs, S, x, dx, ds, gates[0], cs[0], lw[0][1], wx, pw, sw,
                                                  hs[0], dws, nl, persist)
        elif nl > 1 and _one_launch(K.gfront_stack_bwd_ok, T, wx, B, S, fs, nl, dev):
            # the whole loop of ALL layers in ONE launch (ag_gfront_stack_bwd); the stop head's gradient lands on the top layer
            ds_tb = _stop_head_grads(ds, hs[-1].view(T * B, S), dws, 4 * nl + 2, defer=False) if ds is not None else None
            dh_ext, dx_ext = _ext_grads(ds_tb, sw, dx, T, B, S)
            dgs = [torch.empty(T, B, 4 * S, device=dev) for _ in range(nl)]
            dxt = torch.empty(T, B, fs, device=dev)
            K.gfront_stack_bwd_persist(gates, cs, x, dh_ext, dx_ext, [lw[l][1] for l in range(nl)],
                                       [lw[l][0] for l in range(1, nl)], wx, pw, dgs, dxt)
        else:
            dgs, dxt = GFrontFn._bwd_frames(T, B, fs, S, nl, x, dx, ds, gates, cs, lw, wx, pw, sw, hs, dws)
        # parameter gradients, one GEMM per tensor over all frames
        dxt2 = dxt.view(T * B, fs)
        with K.deferred_reduces():      # the bias sums' second stages in ONE launch (read only after the block)
            if wg:
                K.gemm(dxt2, hs[-1].view(T * B, S), dws[4 * nl], ta=True, defer=True)
                K.col_sum(dxt2, dws[4 * nl + 1])
            for l in range(nl if wg else 0):
                dg2 = dgs[l].view(T * B, 4 * S)
                dwih = dws[4 * l]
                if l == 0:
                    K.gemm(dg2, zc.contiguous().view(T * B, Fz), dwih[:, fs:], ta=True, defer=True)
                    if T > 1:
                        K.gemm(dgs[0][1:].view((T - 1) * B, 4 * S), _xprev_rows(x, xt, T, B, fs), dwih[:, :fs], ta=True,
                               defer=True)
                else:
                    K.gemm(dg2, hs[l - 1].view(T * B, S), dwih, ta=True, defer=True)
                if T > 1:
                    K.gemm(dgs[l][1:].view((T - 1) * B, 4 * S), hs[l][:T - 1].view((T - 1) * B, S),
                           dws[4 * l + 1], ta=True, defer=True)
                K.col_sum(dg2, dws[4 * l + 2])
        for l in range(nl if wg else 0):
            dws[4 * l + 3] = dws[4 * l + 2]       # b_hh sees the same gradient as b_ih: the weight-norm backward reads one buffer twice
        dzc = None
        if ctx.needs_input_grad[0]:
            dzc = torch.empty(T * B, Fz, device=dev)
            K.gemm(dgs[0].view(T * B, 4 * S), lw[0][0][:, fs:], dzc)
            dzc = dzc.view(T, B, Fz)
        grads = front.group.backward(dws, ctx.needs_input_grad[2:]) if wg else [None] * (2 * len(front.group.items))
        return (dzc, None) + tuple(grads)


# --------------------------------------------------------------------------------------
# GRU variant of the generator front (BASELINE config C4; oracle = torch.nn.GRUCell because the
# reference has no GRU).  One layer; same frame feedback as GFrontFn.
# --------------------------------------------------------------------------------------
class GRUFront(object):
    """WN items: [w_ih, w_hh, b_ih, b_hh, proj.w, proj.b, stop.w, stop.b]"""

    def __init__(self, frame_size, state_size):
        self.fs, self.ss = frame_size, state_size
        self.slab_channels = 0
        self.group = WNGroup()


class GRUFrontFn(torch.autograd.Function):
    """zc [T,B,Fz] -> x [B,T*fs], s [B,T];  frame t: h_t = GRUCell([x_{t-1}, zc_t], h_{t-1}),
    x_t = tanh(proj(h_t)), s_t = stopper(h_t)."""

    @staticmethod
    def forward(ctx, zc, front, *params):
        T, B, Fz = zc.shape
        fs, S = front.fs, front.ss
        dev = zc.device
        ctx.set_materialize_grads(False)
        w_ih, w_hh, b_ih, b_hh, pw, pb, sw, sb = [p.w for p in front.group.prepare()]
        wx, wz = w_ih[:, :fs], w_ih[:, fs:]
        x = _frames_buffer(front, B, T * fs, dev)
        xt = None
        gi = torch.empty(T, B, 3 * S, device=dev)      # -> activated (r, z, n)
        gh = torch.empty(T, B, 3 * S, device=dev)      # h-part incl. b_hh (n slot needed for backward)
        hs = torch.empty(T + 1, B, S, device=dev)      # hs[t+1] = h_t, hs[0] = 0
        hs[0].zero_()
        if _one_launch(K.gfront_persist_ok, T, wx, B, S, fs, dev):
            # the whole frame loop (GRU step + projection, fed back) in ONE launch, weights resident in registers
            _front_pre(zc, wz, b_ih, b_hh, gi, gru=True)
            xt = torch.empty(T, B, fs, device=dev)
            K.grufront_fwd_persist(gi, gh, wx, w_hh, b_hh[2 * S:].contiguous(), pw, pb, hs[1:], x, xt)
        else:
            GRUFrontFn._fwd_frames(T, B, fs, S, zc, x, gi, gh, hs, wx, wz, w_hh, b_ih, b_hh, pw, pb)
        s = torch.empty(T * B, 1, device=dev)
        _linear1(hs[1:].view(T * B, S), sw, sb, s)
        ctx.front, ctx.key, ctx.dims = front, front.group._key[1:], (T, B, Fz)
        ctx.has_xt = xt is not None
        ctx.save_for_backward(zc, x, gi, gh, hs, *([xt] if xt is not None else []))
        return x, s.view(T, B).t()

    @staticmethod
    def _fwd_frames(T, B, fs, S, zc, x, gi, gh, hs, wx, wz, w_hh, b_ih, b_hh, pw, pb):
        """per-frame chain, one launch per operation; hs[0] = 0 is the caller's"""
        K.gemm(zc.contiguous().view(T * B, zc.size(2)), wz, gi.view(T * B, 3 * S), tb=True, bias=b_ih)
        for t in range(T):
            if t > 0:
                _small_acc(x[:, (t - 1) * fs:t * fs], wx, gi[t], tb=True)
            _small(hs[t], w_hh, gh[t], tb=True, bias=b_hh)
            K.gru_cell_fwd(gi[t], gh[t], hs[t], hs[t + 1])
            _small(hs[t + 1], pw, x[:, t * fs:(t + 1) * fs], tb=True, bias=pb, act=ACT_TANH)

    @staticmethod
    def _bwd_frames(T, B, fs, S, x, dx, ds_tb, gi, gh, hs, w_hh, wx, pw, sw, dgi, dgh, dxt):
        """per-frame chain, one launch per operation, into dgi, dgh and dxt"""
        dev = x.device
        dxa = dx.contiguous().clone() if dx is not None else torch.zeros(B, T * fs, device=dev)
        dha = torch.zeros(T + 1, B, S, device=dev)     # dha[t+1] accumulates dL/dh_t
        if ds_tb is not None:
            K.gemm(ds_tb, sw, dha[1:].view(T * B, S))
        dh_dir = torch.empty(B, S, device=dev)
        for t in reversed(range(T)):
            gx = dxt[t]
            K.act_bwd2d(dxa[:, t * fs:(t + 1) * fs], x[:, t * fs:(t + 1) * fs], gx, ACT_TANH)
            _small_acc(gx, pw, dha[t + 1])
            K.gru_cell_bwd(gi[t], gh[t], hs[t], dha[t + 1], dgi[t], dgh[t], dh_dir)
            K.axpby(dh_dir, dha[t], 1.0, 1.0)                     # direct path  dh * z
            _small_acc(dgh[t], w_hh, dha[t])                      # through the hidden product
            if t > 0:
                _small_acc(dgi[t], wx, dxa[:, (t - 1) * fs:t * fs])

    @staticmethod
    def backward(ctx, dx, ds):
        front = ctx.front
        fs, S = front.fs, front.ss
        T, B, Fz = ctx.dims
        prep = front.group.prepare()
        assert front.group._key[1:] == ctx.key, 'parameters changed between forward and backward'
        w_ih, w_hh, _, _, pw, _, sw, _ = [p.w for p in prep]
        wx = w_ih[:, :fs]
        zc, x, gi, gh, hs = ctx.saved_tensors[:5]
        xt = ctx.saved_tensors[5] if ctx.has_xt else None
        dev = zc.device
        wg = any(ctx.needs_input_grad[2:])
        dws = front.group.zero_dws() if wg else None
        dgi = torch.empty(T, B, 3 * S, device=dev)
        dgh = torch.empty(T, B, 3 * S, device=dev)
        dxt = torch.empty(T, B, fs, device=dev)
        ds_tb = _stop_head_grads(ds, hs[1:].view(T * B, S), dws, 6, defer=False) if ds is not None else None
        if _one_launch(K.gfront_bwd_persist_ok, T, wx, B, S, fs, dev):
            # the whole loop in ONE launch (ag_gfront_bwd)
            dh_ext, dx_ext = _ext_grads(ds_tb, sw, dx, T, B, S)
            K.grufront_bwd_persist(gi, hs, gh, x, dh_ext, dx_ext, w_hh, wx, pw, dgi, dgh, dxt)
        else:
            GRUFrontFn._bwd_frames(T, B, fs, S, x, dx, ds_tb, gi, gh, hs, w_hh, wx, pw, sw, dgi, dgh, dxt)
        dxt2, dgi2, dgh2 = dxt.view(T * B, fs), dgi.view(T * B, 3 * S), dgh.view(T * B, 3 * S)
        if wg:
            K.gemm(dxt2, hs[1:].view(T * B, S), dws[4], ta=True)
            K.col_sum(dxt2, dws[5])
            K.gemm(dgi2, zc.contiguous().view(T * B, Fz), dws[0][:, fs:], ta=True)
            if T > 1:
                K.gemm(dgi[1:].view((T - 1) * B, 3 * S), _xprev_rows(x, xt, T, B, fs), dws[0][:, :fs], ta=True)
            K.gemm(dgh2, hs[:T].view(T * B, S), dws[1], ta=True)
            K.col_sum(dgi2, dws[2])
            K.col_sum(dgh2, dws[3])
        dzc = None
        if ctx.needs_input_grad[0]:
            dzc = torch.empty(T * B, Fz, device=dev)
            K.gemm(dgi2, w_ih[:, fs:], dzc)
            dzc = dzc.view(T, B, Fz)
        return (dzc, None) + tuple(front.group.backward(dws, ctx.needs_input_grad[2:]) if wg else [None] * (2 * len(front.group.items)))


# --------------------------------------------------------------------------------------
# Sampling (Generator.generate): the frame loop with the stop draws, no autograd, no history
# --------------------------------------------------------------------------------------
def first_stops(stops, T):
    """[B,T'] 0/1 draws -> int64 [B]: the frames each clip generates, up to and including its first stop draw (T if none:
    audiogan.py:451-458)"""
    return torch.where(stops.bool().any(1), stops.long().argmax(1) + 1, torch.full_like(stops[:, 0].long(), T))


def front_sample(front, zc, u):
    """the frame loop of a sample (``GFront`` or ``GRUFront``): zc [T,B,Fz] contiguous, u [T,B] uniforms; clip b stops at frame
    t when u[t,b] < sigmoid(s[b,t]) (the reference's Bernoulli draw, :450).  Returns (x [B, T*fs], s [B,T], first int64 [B])
    where first[b] = the frames clip b generates; only the first max(first) frames of x and s are meaningful.

    Where a persistent launch fits (one layer: ag_gfront_fwd at a supported (B, S, fs); 2 to 8 LSTM layers: ag_gfront_stack_fwd
    at a supported (B, S, fs, nl)): ONE launch (gen = 1), which draws the stops itself, keeps no history and leaves its frame
    loop one frame after every clip has stopped.  Otherwise the training front runs under no_grad, same rule on its logits."""
    T, B, Fz = zc.shape
    fs, S = front.fs, front.ss
    gru = isinstance(front, GRUFront)
    nl = 1 if gru else front.nl
    dev = zc.device
    prep = front.group.prepare()
    w_ih, w_hh, b_ih, b_hh = [p_.w for p_ in prep[:4]]
    pw, pb, sw, sb = [p_.w for p_ in prep[4 * nl:4 * nl + 4]]
    wx, wz = w_ih[:, :fs], w_ih[:, fs:]
    stack = nl > 1 and _one_launch(K.gfront_stack_ok, T, wx, B, S, fs, nl, dev)
    if stack or (nl == 1 and _one_launch(K.gfront_persist_ok, T, wx, B, S, fs, dev)):
        pre = torch.empty(T, B, (3 if gru else 4) * S, device=dev)
        _front_pre(zc, wz, b_ih, b_hh, pre, gru)
        x = _frames_buffer(front, B, T * fs, dev)
        s = torch.empty(B, T, device=dev)
        first = torch.empty(B, dtype=torch.int32, device=dev)
        t_run = torch.empty(1, dtype=torch.int32, device=dev)
        if stack:
            # a stacked front: ONE ag_gfront_stack_fwd launch (gen = 1); the top layer's h feeds the projection and the stop head
            lw = [[p_.w for p_ in prep[4 * l:4 * l + 4]] for l in range(nl)]
            K.gfront_stack_gen_persist(pre, wx, [lw[l][0] for l in range(1, nl)], [lw[l][1] for l in range(nl)],
                                       [lw[l][2] + lw[l][3] for l in range(1, nl)], pw, pb, sw.view(-1), sb, u.contiguous(),
                                       x, s, first, t_run)
        else:
            K.gfront_gen_persist(pre, wx, w_hh, pw, pb, sw.view(-1), sb, u.contiguous(), x, s, first, t_run,
                                 bhn=b_hh[2 * S:].contiguous() if gru else None)
        return x, s, first.long(), t_run
    with torch.no_grad():
        x, s = (GRUFrontFn if gru else GFrontFn).apply(zc, front, *front.group.params())
    return x, s, first_stops(u.t() < torch.sigmoid(s), T), None

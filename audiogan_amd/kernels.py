"""Tensor-level wrappers over the C ABI (include/audiogan_hip.h).

Every function takes torch CUDA fp32 tensors (views allowed where noted), checks what
the kernels assume (device, dtype, unit stride on the last axis, shapes) and enqueues
the kernel on torch's current HIP stream.  Nothing here computes on the host and there
is no fallback: a non-CUDA tensor raises."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_LEAKY_GATE, OPT_RMSPROP, OPT_ADAM  # noqa: F401

LEAKY_SLOPE = 0.01


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


BF16 = torch.bfloat16
_F32_OR_BF16 = (torch.float32, torch.bfloat16)      # a ``dtype`` of _chk / _mat / a check-table row: either storage type


def _chk(t, name, dtype=torch.float32):
    """a device tensor of ``dtype`` (one dtype, or a tuple of the allowed ones); None - an optional tensor - passes"""
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError('audiogan_amd: %s must be a CUDA (HIP) tensor; there is no CPU path' % name)
    if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        want = ' or '.join(str(d_) for d_ in dtype) if isinstance(dtype, tuple) else dtype
        raise TypeError('audiogan_amd: %s must be %s, got %s' % (name, want, t.dtype))


def _is16(t):
    return t is not None and t.dtype == torch.bfloat16


# bf16 STORAGE (BASELINE configs[2], round 4): in 'bf16' precision mode the critic's sequence path keeps its activations,
# their gradients and the GEMM operands as bfloat16 in HBM (ag_gemm_h reads them straight into LDS); fp32 accumulators,
# master weights, gate pre-activations / cell states of the recurrent kernels and optimiser state are unchanged.
# AG_BF16_STORE=0 keeps the round-3 form (fp32 in memory, rounded per use) for A/B runs.
BF16_STORE = [os.environ.get('AG_BF16_STORE', '1') != '0']


def bf16_storage():
    return BF16_STORE[0] and lib.ag_get_precision() == 1


def _bcl(t, name):
    """(batch stride, channel stride) of a [B,C,L] view with unit time stride."""
    _chk(t, name)
    if t.dim() != 3 or (t.size(2) > 1 and t.stride(2) != 1):
        raise ValueError('audiogan_amd: %s must be [B,C,L] with unit stride along L' % name)
    return t.stride(0), t.stride(1)


def _mat(t, name, dtype=torch.float32):
    """leading dimension of a 2-D row-major view"""
    _chk(t, name, dtype)
    if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
        raise ValueError('audiogan_amd: %s must be 2-D with unit stride along dim 1' % name)
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


# ------------------------------------------------------------------------------------
# two-stage (deterministic) reductions: a per-call workspace bound right before the C call
# ------------------------------------------------------------------------------------
_SMALL_WS = 1 << 17        # floats; enough for the bias / channel / column sums at every BASELINE size


# process-wide, like the C side (api.hip): a scope is opened by the thread that calls loss.backward() and the recording
# calls come from torch's autograd thread (never concurrently: the opener blocks inside backward())
#   keep   workspaces kept alive until the flush (None: no scope)
#   outer  the scope was opened by a network-level caller (common.network_backward): it RECORDS only inside the inner
#          ``deferred_reduces()`` blocks of the autograd Functions (each block vouches that nothing inside it reads the
#          sums it defers) and flushes once, when the whole backward is over
#   depth  inner blocks currently open
_DEFER = dict(keep=None, outer=False, depth=0)


def reduces_recording():
    return _DEFER['keep'] is not None and (_DEFER['depth'] > 0 or not _DEFER['outer'])


def reduces_outer():
    """is a network-level scope open?  (its sums are final only when IT closes: see common.WNGroup.backward)"""
    return _DEFER['keep'] is not None and _DEFER['outer']


class deferred_reduces(object):
    """``with K.deferred_reduces(): ...`` - the second stages of every two-stage reduction issued inside (conv weight
    gradients, bias / channel / column sums, split-K weight-gradient GEMMs called with ``defer=True``) run as ONE launch at
    the end instead of one each (ag_defer_reduces / ag_flush_reduces; same results bit for bit).  Nothing inside the block
    may read those outputs.  The partial-sum workspaces are kept alive until the flush.
    A reducing call that writes at once into floats a recorded stage still has to write (a single-writer form, a
    ``defer=False`` call) sums the recorded stages first, so one destination sees its writes in the order of the calls.
    Kernels outside the reducing family (axpby, torch's own zero_, ...) remain the caller's business: flush_reduces() first.
    ``outer=True`` (common.network_backward): open a scope around a whole backward pass; it records only inside the
    Functions' own ``deferred_reduces()`` blocks, and those blocks then do NOT flush when they end - everything recorded
    by the whole backward is summed by one launch when the outer scope closes."""

    def __init__(self, outer=False):
        self.outer = bool(outer)
        self.role = None

    def __enter__(self):
        st = _DEFER
        if st['keep'] is None:
            check(lib.ag_defer_reduces(1), 'ag_defer_reduces')
            st['keep'], st['outer'], st['depth'] = [], self.outer, 0
            self.role = 'owner'
            if self.outer:
                lib.ag_defer_reduces(2)                # paused until an inner block opens
        elif self.outer:
            self.role = 'nested'                       # a network scope inside another scope: the outermost one rules
        else:
            if st['outer'] and st['depth'] == 0:
                check(lib.ag_defer_reduces(3), 'ag_defer_reduces')
            st['depth'] += 1
            self.role = 'inner'
        return self

    def __exit__(self, et, ev, tb):
        st = _DEFER
        if self.role == 'inner':
            st['depth'] -= 1
            if st['outer'] and st['depth'] == 0:
                lib.ag_defer_reduces(2)
        elif self.role == 'owner':
            try:
                if et is None:
                    check(lib.ag_flush_reduces(_stream()), 'ag_flush_reduces')
            finally:
                st['keep'], st['outer'], st['depth'] = None, False, 0
                lib.ag_defer_reduces(1)        # drops whatever is still recorded (error path) ...
                lib.ag_defer_reduces(0)        # ... and turns deferral off
        return False


def flush_reduces():
    """sum everything recorded so far NOW (a reader inside a scope needs final values); the scope stays open"""
    if _DEFER['keep'] is not None:
        check(lib.ag_flush_reduces(_stream()), 'ag_flush_reduces')


class _immediate(object):
    """the reducing call inside runs its second stage at once even inside a recording scope"""

    def __enter__(self):
        self.on = reduces_recording()
        if self.on:
            lib.ag_defer_reduces(2)

    def __exit__(self, *exc):
        if self.on:
            lib.ag_defer_reduces(3)


def _bind_ws(numel, dev):
    """bind `numel` floats of scratch for the NEXT reducing call (ag_bind_workspace); the tensor comes from torch's
    stream-ordered caching allocator, so it is safe to drop it as soon as the call has been enqueued"""
    if numel <= 0:
        lib.ag_bind_workspace(None, 0)       # no workspace for this call: drop whatever an earlier, failed call left bound
        return None
    ws = torch.empty(int(numel), dtype=torch.float32, device=dev)
    check(lib.ag_bind_workspace(_p(ws), int(numel)), 'ag_bind_workspace')
    if _DEFER['keep'] is not None:
        _DEFER['keep'].append(ws)
    return ws


# ------------------------------------------------------------------------------------
# precision mode of the contractions (ag_set_precision): 'f32' (default) or 'bf16'
# ------------------------------------------------------------------------------------
def set_precision(mode):
    """'f32': exact fp32 contractions.  'bf16': every contraction rounds both operands to bfloat16 (RNE) and
    accumulates in fp32 (GEMMs and the persistent recurrent kernels on v_mfma_f32_32x32x16_bf16 / rounded operands);
    memory, epilogues, losses and the optimiser stay fp32.  Returns the previous mode."""
    old = get_precision()
    check(lib.ag_set_precision({'f32': 0, 'bf16': 1, 'f32x3': 2}[mode]), 'ag_set_precision')
    return old


def get_precision():
    """'f32x3' is an experiment (bench.py --dtype f32x3): the large GEMMs on three bf16 MFMAs per product of bf16 hi + lo
    operand parts (~2^-16 relative per product), everything else exact fp32"""
    return {0: 'f32', 1: 'bf16', 2: 'f32x3'}[lib.ag_get_precision()]


class precision(object):
    """``with K.precision('bf16'): ...``"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = set_precision(self.mode)
        return self

    def __exit__(self, *exc):
        set_precision(self.old)


def wpa_numel(d0, d1, K):
    return int(lib.ag_wpa_numel(d0, d1, K))


def wpb_numel(d0, d1, K, stride):
    return int(lib.ag_wpb_numel(d0, d1, K, stride))


# ------------------------------------------------------------------------------------
# descriptor tables (device copies of small C struct arrays), cached by content
# ------------------------------------------------------------------------------------
_table_cache = OrderedDict()     # descriptor tables created eagerly: LRU, bounded
_table_pinned = {}               # tables created while a hipGraph was being captured: the graph's copy node re-reads
                                 # the pinned slot and its kernels read the device table on every replay - never evicted
_TABLE_LRU = 4096


def _table(kind, structs, device):
    raw = b''.join(bytes(s) for s in structs)
    key = (kind, raw, str(device))
    t = _table_pinned.get(key)
    if t is not None:
        return t[0]
    capturing = torch.device(device).type == 'cuda' and torch.cuda.is_current_stream_capturing()
    t = _table_cache.get(key)
    if t is not None:
        if capturing:
            # uploaded eagerly before the capture began (complete: capture starts behind a synchronize): the graph's
            # kernels may read it as it is, without a copy node - but from now on it must never be evicted
            _table_pinned[key] = _table_cache.pop(key)
            _capture_log.append(key)
            return t[0]
        _table_cache.move_to_end(key)
        return t[0]
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    if torch.device(device).type == 'cuda':
        # staged through a pre-allocated pinned arena + async copy: legal inside hipGraph capture (the copy becomes a
        # graph node that re-reads the arena slot on replay, so slots are never recycled)
        host = _pinned_slot(len(raw))
        host.copy_(src)
        t = torch.empty(len(raw), dtype=torch.uint8, device=device)
        t.copy_(host, non_blocking=True)
    else:
        host, t = src, src.to(device)
    if capturing:
        _table_pinned[key] = (t, host)
        _capture_log.append(key)
        TABLE_STATS['uploads_in_capture'] += 1
        TABLE_STATS['kinds'].append(kind)
    else:
        _table_cache[key] = (t, host)
        while len(_table_cache) > _TABLE_LRU:
            _table_cache.popitem(last=False)
    return t


_capture_log = []
# descriptor tables that had to be UPLOADED by a copy node of a captured graph (their content was not seen by an eager step
# before the capture): each costs a ~5 us node per replay - bench.py reports the count
TABLE_STATS = dict(uploads_in_capture=0, kinds=[])


def capture_mark():
    """position in the log of tables created under capture (see drop_captured_tables)"""
    return len(_capture_log)


def drop_captured_tables(mark):
    """forget the tables created under a capture that FAILED or will never be replayed (their device content was
    never written): call with the capture_mark() taken before the capture started"""
    while len(_capture_log) > mark:
        _table_pinned.pop(_capture_log.pop(), None)


_arena = {'buf': None, 'off': 0}


def _pinned_slot(nbytes):
    n = (nbytes + 63) // 64 * 64
    a = _arena
    if a['buf'] is None or a['off'] + n > a['buf'].numel():
        a['buf'] = torch.empty(max(4 << 20, n), dtype=torch.uint8).pin_memory()
        a['off'] = 0
    s = a['buf'][a['off']:a['off'] + n]
    a['off'] += n
    return s[:nbytes]


def reserve_table_arena():
    """allocate the pinned staging arena now (call before hipGraph capture)"""
    if _arena['buf'] is None:
        _pinned_slot(64)


# ------------------------------------------------------------------------------------
# per-kernel timing hook for bench.py's roofline figure: HIP events recorded on the launch
# stream around the launches of ONE kernel class (or all of them in the discovery pass).
# A wrapper is timed iff its ``def`` carries ``@_timed(...)``; its work model stands right above it.
# ------------------------------------------------------------------------------------
class Profiler(object):
    enabled = False
    only = None          # kernel name (as ag_last_kernel / rocprofv3 spell it) or class key to time, or None = all
    records = []         # (key, flops, bytes, ev_start, ev_stop)

    @classmethod
    def start(cls, only=None):
        cls.enabled, cls.only, cls.records = True, only, []

    @classmethod
    def stop(cls):
        cls.enabled = False
        torch.cuda.synchronize()
        out = {}
        for key, fl, by, e0, e1, nl in cls.records:
            r = out.setdefault(key, dict(n=0, ms=0.0, flops=0.0, bytes=0.0))
            r['n'] += nl
            r['ms'] += e0.elapsed_time(e1)
            r['flops'] += fl
            r['bytes'] += by
        cls.records = []
        return out


def _bf16_tag():
    """bf16 mode: the persistent recurrent kernels run their v_mfma_f32_*_bf16 instantiation"""
    return '<bf16>' if lib.ag_get_precision() == 1 else ''


def _call_sig(a, k):
    """everything about a call that a dispatch rule could look at, without knowing any rule: per argument a tensor's shape,
    strides, dtype and alignment, a list element by element, anything else by value; plus the precision mode.  The result
    is a dict key: every other argument must be hashable (numbers, bools, None, strings - all the four naming wrappers take)"""
    def one(v):
        if isinstance(v, torch.Tensor):
            return tuple(v.shape), v.stride(), v.dtype, v.data_ptr() % 16
        if isinstance(v, (list, tuple)):
            return tuple(one(e) for e in v)
        return v
    return tuple(one(v) for v in a), tuple((n, one(k[n])) for n in sorted(k)), lib.ag_get_precision()


def _timed(work=None, name=None):
    """``@_timed(work)`` on a wrapper's ``def``: under the Profiler its calls are timed and filed.  ``work``: a model
    _work_*(same arguments as the wrapped call) -> (key, flops, bytes[, launches]), the algorithmic work of the call from its
    shapes; key None: the library chose among kernel forms and names the one it launched itself (ag_last_kernel).  No
    model: filed under ``name`` (default: the function's own) with no work.  The wrapper shows both as ``timed_work`` and
    ``timed_name`` (tests/test_launch_layer.py pins the whole set)."""
    def deco(fn):
        me = name or fn.__name__
        seen = {}       # call signature -> the kernel name the library reported for it last time (only steers `only`)

        def wrapped(*a, **k):
            if not Profiler.enabled:
                return fn(*a, **k)
            w_ = work(*a, **k) if work is not None else (me, 0.0, 0.0)
            key, fl, by = w_[:3]
            nl = w_[3] if len(w_) > 3 else 1        # launches behind this call (a whole recurrent layer pass: T)
            only = Profiler.only
            if key is None:
                sig = _call_sig(a, k)
                if only is not None and seen.get(sig, only) != only:     # (a signature not seen yet is timed and learnt)
                    return fn(*a, **k)
            elif only is not None and key != only:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            if key is None:
                key = seen[sig] = lib.ag_last_kernel().decode()
            Profiler.records.append((key, fl, by, e0, e1, nl))
            return r
        wrapped.__name__ = me
        wrapped.__doc__ = fn.__doc__
        wrapped.__module__ = __name__
        wrapped.timed_work, wrapped.timed_name = work, me
        return wrapped
    return deco


def _work_named(*a_, **kw):
    """(filed under the name the launch site reported: ag_last_kernel)"""
    return None, 0.0, 0.0


# ------------------------------------------------------------------------------------
# weight norm
# ------------------------------------------------------------------------------------
@_timed()
def weight_norm_fwd(entries):
    """entries: list of dict(v, g, w=None, wpa=None, wpb=None, stride=1, pad=0).  v is the
    parameter tensor ([d0], [d0,d1] or [d0,d1,K]); outputs are written in place.  ``pad``: the conv padding the
    scatter layout wpb is prepared for (aligned layout, see conv_engine's wp_pad)."""
    descs, max_rows = [], 1
    for e in entries:
        v, g = e['v'], e['g']
        _chk(v, 'v'); _chk(g, 'g')
        assert v.is_contiguous() and g.is_contiguous() and g.numel() == v.size(0)
        rows = v.size(0)
        cols = v.numel() // rows
        if v.dim() == 3:
            d1, K = v.size(1), v.size(2)
        else:
            d1, K = cols, 1
        for k in ('w', 'wpa', 'wpb'):
            _chk(e.get(k), k)
        if e.get('w') is not None:
            assert e['w'].is_contiguous() and e['w'].numel() == v.numel()
        s = int(e.get('stride', 1))
        if e.get('wpa') is not None:
            assert e['wpa'].numel() == wpa_numel(rows, d1, K)
        if e.get('wpb') is not None:
            assert e['wpb'].numel() == wpb_numel(rows, d1, K, s)
        descs.append(_lib.WnDesc(v.data_ptr(), g.data_ptr(), _p(e.get('w')).value or 0,
                                 _p(e.get('wpa')).value or 0, _p(e.get('wpb')).value or 0, 0,
                                 rows, cols, d1, K, s, int(e.get('pad', 0))))
        max_rows = max(max_rows, rows)
    tab = _table('wn', descs, entries[0]['v'].device)
    check(lib.ag_weight_norm_fwd(_p(tab), len(descs), max_rows, _stream()), 'ag_weight_norm_fwd')


@_timed()
def weight_norm_bwd(entries):
    """entries: list of dict(v, g, dw, dv, dg[, accumulate]); dv/dg are written (or added to)."""
    descs, max_rows = [], 1
    for e in entries:
        for k in ('v', 'g', 'dw', 'dv', 'dg'):
            _chk(e[k], k)
            assert e[k].is_contiguous()
        rows = e['v'].size(0)
        cols = e['v'].numel() // rows
        assert e['dw'].numel() == e['v'].numel() == e['dv'].numel() and e['dg'].numel() == rows
        descs.append(_lib.WnBwdDesc(e['v'].data_ptr(), e['g'].data_ptr(), e['dw'].data_ptr(),
                                    e['dv'].data_ptr(), e['dg'].data_ptr(), rows, cols,
                                    1 if e.get('accumulate') else 0, 0))
        max_rows = max(max_rows, rows)
    tab = _table('wnb', descs, entries[0]['v'].device)
    check(lib.ag_weight_norm_bwd(_p(tab), len(descs), max_rows, _stream()), 'ag_weight_norm_bwd')


def prep_conv_weight(w, wpa, wpb, stride, pad=0):
    _chk(w, 'w'); _chk(wpa, 'wpa'); _chk(wpb, 'wpb')
    assert w.dim() == 3 and w.is_contiguous()
    d0, d1, K = w.shape
    if wpa is not None:
        assert wpa.numel() == wpa_numel(d0, d1, K)
    if wpb is not None:
        assert wpb.numel() == wpb_numel(d0, d1, K, stride)
    check(lib.ag_prep_conv_weight(_p(w), _p(wpa), _p(wpb), d0, d1, K, stride, int(pad), _stream()),
          'ag_prep_conv_weight')


# ------------------------------------------------------------------------------------
# conv engine
# ------------------------------------------------------------------------------------
def _work_conv(x, wp, y, K_, stride, pad, mode, *a_, **kw):
    B, Cc, Lin = x.shape
    _, O, Lout = y.shape
    macs = B * O * Lout * Cc * K_ if mode == 0 else B * Cc * Lin * O * K_
    return None, 2.0 * macs, 4.0 * (x.numel() + y.numel() + O * Cc * K_)


@_timed(_work_conv)
def conv_engine(x, wp, y, K, stride, pad, mode, bias=None, res=None, lens=None, act=ACT_NONE,
                slope=LEAKY_SLOPE, accumulate=False, wp_pad=0):
    """mode 0: y[b,o,t] = sum W x[b,c,s*t+k-p]   (wp = gather layout of the weight)
    mode 1: y[b,o,s*t+k-p] += W x[b,c,t]        (wp = scatter layout; wp_pad = the padding it was prepared for)
    x: [B,C,Lin] view, y: [B,O,Lout] view (written in place).  act=ACT_LEAKY_GATE: ``res`` is the saved output of a
    LeakyReLU and scales the result by that activation's derivative instead of being added."""
    assert act != ACT_LEAKY_GATE or res is not None, 'ACT_LEAKY_GATE needs the saved activation in `res`'
    x_bs, x_cs = _bcl(x, 'x')
    y_bs, y_cs = _bcl(y, 'y')
    _chk(wp, 'wp'); _chk(bias, 'bias'); _chk(lens, 'lens', torch.int64)
    B, Cc, Lin = x.shape
    B2, O, Lout = y.shape
    assert B == B2
    if mode == 0:
        assert wp.numel() == wpa_numel(O, Cc, K), 'gather weight layout does not match shapes'
    else:
        assert wp.numel() == wpb_numel(Cc, O, K, stride), 'scatter weight layout does not match'
    r_bs = r_cs = 0
    if res is not None:
        r_bs, r_cs = _bcl(res, 'res')
        assert tuple(res.shape) == tuple(y.shape)
    if bias is not None:
        assert bias.numel() == O and bias.is_contiguous()
    if lens is not None:
        assert lens.numel() == B and lens.is_contiguous()
    a = _lib.ConvArgs(x.data_ptr(), wp.data_ptr(), _p(bias).value or 0, _p(res).value or 0,
                      y.data_ptr(), _p(lens).value or 0, x_bs, x_cs, y_bs, y_cs, r_bs, r_cs,
                      B, Cc, Lin, O, Lout, K, stride, pad, mode, act, slope, 1 if accumulate else 0, int(wp_pad))
    check(lib.ag_conv1d_engine(C.byref(a), _stream()), 'ag_conv1d_engine')


def _work_wgrad(sh, lg, dw, K_, stride, pad):
    B, A, Lsh = sh.shape
    Cc = lg.size(1)
    return None, 2.0 * B * A * Lsh * Cc * K_, 4.0 * (sh.numel() + lg.numel() + dw.numel())


@_timed(_work_wgrad)
def conv_wgrad(sh, lg, dw, K, stride, pad):
    """dw[a,c,k] += sum_{b,t} sh[b,a,t] * lg[b,c,s*t+k-p];  dw: [A,C,K] contiguous."""
    sh_bs, sh_cs = _bcl(sh, 'sh')
    lg_bs, lg_cs = _bcl(lg, 'lg')
    _chk(dw, 'dw')
    B, A, Lsh = sh.shape
    B2, Cc, Llg = lg.shape
    assert B == B2 and dw.is_contiguous() and dw.numel() == A * Cc * K
    _ws = _bind_ws(lib.ag_conv1d_wgrad_ws_numel(B, A, Lsh, Cc, K), dw.device)  # noqa: F841
    check(lib.ag_conv1d_wgrad(_p(sh), sh_bs, sh_cs, _p(lg), lg_bs, lg_cs, _p(dw), B, A, Lsh, Cc, Llg,
                              K, stride, pad, _stream()), 'ag_conv1d_wgrad')


@_timed()
def channel_sum(dy, db, accumulate=True):
    """db[c] (+)= sum_{b,t} dy[b,c,t]"""
    bs, cs = _bcl(dy, 'dy')
    _chk(db, 'db')
    B, Cc, L = dy.shape
    assert db.numel() == Cc and db.is_contiguous()
    _ws = _bind_ws(_SMALL_WS, db.device)  # noqa: F841
    check(lib.ag_channel_sum(_p(dy), bs, cs, _p(db), B, Cc, L, int(bool(accumulate)), _stream()), 'ag_channel_sum')


@_timed()
def leaky_bwd(dy, y, dpre, lens=None, slope=LEAKY_SLOPE, add_into=None, bias_grad=None):
    """dpre = dy * (y > 0 ? 1 : slope) * (t < lens[b]); all [B,C,L] views; dpre may alias dy.
    add_into (optional [B,C,L] view, must not overlap dpre): add_into += dpre.
    bias_grad (optional [C], pre-zeroed): bias_grad[c] += sum_{b,t} dpre[b,c,t]."""
    a = _bcl(dy, 'dy'); b = _bcl(y, 'y'); c = _bcl(dpre, 'dpre')
    d = _bcl(add_into, 'add_into') if add_into is not None else (0, 0)
    _chk(lens, 'lens', torch.int64)
    assert tuple(dy.shape) == tuple(y.shape) == tuple(dpre.shape)
    assert add_into is None or tuple(add_into.shape) == tuple(dy.shape)
    B, Cc, L = dy.shape
    if bias_grad is not None:
        _chk(bias_grad, 'bias_grad')
        assert bias_grad.is_contiguous() and bias_grad.numel() == Cc
        _ws = _bind_ws(_SMALL_WS, bias_grad.device)  # noqa: F841
    check(lib.ag_leaky_bwd(_p(dy), a[0], a[1], _p(y), b[0], b[1], _p(dpre), c[0], c[1], _p(add_into),
                           d[0], d[1], _p(lens), _p(bias_grad), B, Cc, L, slope, _stream()), 'ag_leaky_bwd')


# ------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------
def _work_gemm(A, B, Cm, ta=False, tb=False, *a_, **kw):
    M, N = Cm.shape
    Kd = A.size(0) if ta else A.size(1)
    return None, 2.0 * M * N * Kd, 4.0 * (M * Kd + N * Kd + M * N)


@_timed(_work_gemm)
def gemm(A, B, Cm, ta=False, tb=False, alpha=1.0, beta=0.0, bias=None, res=None, act=ACT_NONE,
         slope=LEAKY_SLOPE, defer=False):
    """Cm[M,N] = act(alpha * op(A) @ op(B) + beta*Cm + bias + res).
    ta: A is stored [K,M];  tb: B is stored [N,K] (a Linear weight).
    ``defer``: Cm is a parameter gradient that nothing reads before the enclosing ``deferred_reduces`` scope closes - a
    split-K product may then leave its second stage to the scope's one launch.  Default: the product is complete when the
    call returns (in stream order), also inside a scope."""
    lda, ldb, ldc = _mat(A, 'A'), _mat(B, 'B'), _mat(Cm, 'C')
    M, N = Cm.shape
    K = A.size(0) if ta else A.size(1)
    assert (A.size(1) if ta else A.size(0)) == M, 'gemm: A shape'
    assert (B.size(1) if tb else B.size(0)) == K and (B.size(0) if tb else B.size(1)) == N, 'gemm: B shape'
    ldres = 0
    if res is not None:
        ldres = _mat(res, 'res')
        assert tuple(res.shape) == (M, N)
    if bias is not None:
        _chk(bias, 'bias')
        assert bias.numel() == N and bias.is_contiguous()
    nws = lib.ag_gemm_ws_numel(M, N, K, act)
    hold = (not defer) and nws > 0 and reduces_recording()
    if hold:
        lib.ag_defer_reduces(2)
    try:
        _ws = _bind_ws(nws, Cm.device)  # noqa: F841
        check(lib.ag_gemm(_p(A), lda, int(ta), _p(B), ldb, int(tb), _p(Cm), ldc, M, N, K, alpha, beta,
                          _p(bias), _p(res), ldres, act, slope, _stream()), 'ag_gemm')
    finally:
        if hold:
            lib.ag_defer_reduces(3)


@_timed()
def col_sum(X, out, accumulate=True, defer=True):
    """out[n] (+)= sum_m X[m,n].  ``defer=False``: complete when the call returns (in stream order) also inside a recording
    ``deferred_reduces`` scope - for sums that are read before that scope closes."""
    ldx = _mat(X, 'X', _F32_OR_BF16)
    _chk(out, 'out')
    M, N = X.shape
    assert out.numel() == N and out.is_contiguous()
    hold = (not defer) and reduces_recording()
    if hold:
        lib.ag_defer_reduces(2)
    try:
        _ws = _bind_ws(min(_SMALL_WS, 64 * N) if M > 16 else 0, out.device)  # noqa: F841
        check(lib.ag_col_sum(_p(X), int(_is16(X)), ldx, _p(out), M, N, int(bool(accumulate)), _stream()), 'ag_col_sum')
    finally:
        if hold:
            lib.ag_defer_reduces(3)


# ------------------------------------------------------------------------------------
# LSTM cell pointwise
# ------------------------------------------------------------------------------------
@_timed()
def lstm_cell_fwd(gates, c_prev, c_out, h_out=None, y_out=None, h_prev=None, valid=None, t=0):
    ldg = _mat(gates, 'gates')
    B, H4 = gates.shape
    H = H4 // 4
    _chk(valid, 'valid', torch.int64)
    ld = lambda x, n: (_mat(x, n) if x is not None else 0)  # noqa: E731
    for x in (c_prev, c_out, h_out, y_out, h_prev):
        assert x is None or tuple(x.shape) == (B, H)
    check(lib.ag_lstm_cell_fwd(_p(gates), ldg, _p(c_prev), ld(c_prev, 'c_prev'), _p(h_out),
                               ld(h_out, 'h_out'), _p(c_out), ld(c_out, 'c_out'), _p(y_out),
                               ld(y_out, 'y_out'), _p(h_prev), ld(h_prev, 'h_prev'), _p(valid), t, B, H,
                               _stream()), 'ag_lstm_cell_fwd')


@_timed()
def lstm_cell_bwd(gates_act, c_prev, c_new, dh, dy, dc_next, dgates, dc_prev, dh_pass=None,
                  valid=None, t=0):
    """dh: gradient from later steps (or None), dy: gradient of this step's output (or None)"""
    B, H4 = gates_act.shape
    H = H4 // 4
    _chk(valid, 'valid', torch.int64)
    ld = lambda x, n: (_mat(x, n) if x is not None else 0)  # noqa: E731
    for x in (c_prev, c_new, dh, dy, dc_next, dc_prev, dh_pass):
        assert x is None or tuple(x.shape) == (B, H)
    assert tuple(dgates.shape) == (B, H4)
    check(lib.ag_lstm_cell_bwd(_p(gates_act), _mat(gates_act, 'gates_act'), _p(c_prev),
                               ld(c_prev, 'c_prev'), _p(c_new), ld(c_new, 'c_new'), _p(dh), ld(dh, 'dh'),
                               _p(dy), ld(dy, 'dy'), _p(dc_next), ld(dc_next, 'dc_next'), _p(dgates), _mat(dgates, 'dgates'),
                               _p(dc_prev), ld(dc_prev, 'dc_prev'), _p(dh_pass), ld(dh_pass, 'dh_pass'),
                               _p(valid), t, B, H, _stream()), 'ag_lstm_cell_bwd')


# ------------------------------------------------------------------------------------
# BCE / activations
# ------------------------------------------------------------------------------------
@_timed()
def bce_logits_fwd(x, target, nframes, per_sample, loss, scale):
    """per_sample[b] = masked sum; loss[0] += scale * sum_b per_sample[b]/n[b]"""
    ldx = _mat(x, 'x')
    _chk(nframes, 'nframes', torch.int64); _chk(per_sample, 'per_sample'); _chk(loss, 'loss')
    B, T = x.shape
    check(lib.ag_bce_logits_fwd(_p(x), ldx, float(target), _p(nframes), _p(per_sample), _p(loss),
                                float(scale), B, T, _stream()), 'ag_bce_logits_fwd')


@_timed()
def bce_logits_bwd(x, target, nframes, gscale, scale, dx):
    ldx, lddx = _mat(x, 'x'), _mat(dx, 'dx')
    _chk(nframes, 'nframes', torch.int64); _chk(gscale, 'gscale')
    B, T = x.shape
    check(lib.ag_bce_logits_bwd(_p(x), ldx, float(target), _p(nframes), _p(gscale), float(scale),
                                _p(dx), lddx, B, T, _stream()), 'ag_bce_logits_bwd')


def bce_logits_fwd_strided(x, target, nframes, per_sample, loss, scale, target_rows=None):
    """x [B,T] of any strides; per_sample[b] = masked sum (optional); loss[0] = scale * sum_b per_sample[b]/n[b] (written);
    target_rows: optional [B] targets (else `target` for every row)"""
    _chk(x, 'x'); _chk(nframes, 'nframes', torch.int64); _chk(per_sample, 'per_sample'); _chk(loss, 'loss')
    _chk(target_rows, 'target_rows')
    B, T = x.shape
    assert target_rows is None or (target_rows.is_contiguous() and target_rows.numel() == B)
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    assert per_sample is None or (per_sample.is_contiguous() and per_sample.numel() == B)
    check(lib.ag_bce_logits_fwd_strided(_p(x), x.stride(0), x.stride(1), float(target), _p(target_rows), _p(nframes),
                                        _p(per_sample), _p(loss), float(scale), B, T, _stream()), 'ag_bce_logits_fwd_strided')


def bce_logits_bwd_strided(x, target, nframes, gscale, scale, dx, target_rows=None):
    _chk(x, 'x'); _chk(dx, 'dx'); _chk(nframes, 'nframes', torch.int64); _chk(gscale, 'gscale'); _chk(target_rows, 'target_rows')
    B, T = x.shape
    assert tuple(dx.shape) == (B, T)
    check(lib.ag_bce_logits_bwd_strided(_p(x), x.stride(0), x.stride(1), float(target), _p(target_rows), _p(nframes),
                                        _p(gscale), float(scale), _p(dx), dx.stride(0), dx.stride(1), B, T, _stream()),
          'ag_bce_logits_bwd_strided')


@_timed()
def act_fwd(x, y, act, slope=LEAKY_SLOPE):
    _chk(x, 'x'); _chk(y, 'y')
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    check(lib.ag_act_fwd(_p(x), _p(y), x.numel(), act, slope, _stream()), 'ag_act_fwd')


@_timed()
def act_bwd(dy, y, dx, act, slope=LEAKY_SLOPE):
    for t_, n in ((dy, 'dy'), (y, 'y'), (dx, 'dx')):
        _chk(t_, n)
        assert t_.is_contiguous()
    assert dy.numel() == y.numel() == dx.numel()
    check(lib.ag_act_bwd(_p(dy), _p(y), _p(dx), dy.numel(), act, slope, _stream()), 'ag_act_bwd')


def bct_to_tbc(x, out=None, out_dtype=None):
    """[B,C,T] (any batch / channel pitch, time contiguous) -> contiguous [T,B,C] (ag_transpose_batched); fp32 or bf16 on
    either side (``out_dtype``: default = x's)"""
    _chk(x, 'x', _F32_OR_BF16)
    B, Cc, T = x.shape
    assert x.stride(2) == 1
    if out is None:
        out = torch.empty(T, B, Cc, device=x.device, dtype=out_dtype or x.dtype)
    _chk(out, 'out', _F32_OR_BF16)
    check(lib.ag_transpose_batched(_p(x), int(_is16(x)), x.stride(0), x.stride(1), _p(out), int(_is16(out)), Cc, B * Cc, B, Cc,
                                   T, _stream()), 'ag_transpose_batched')
    return out


def tbc_to_bct(x, out=None, out_dtype=None):
    """contiguous [T,B,C] -> contiguous [B,C,T] (ag_transpose_batched); fp32 or bf16 on either side"""
    _chk(x, 'x', _F32_OR_BF16)
    T, B, Cc = x.shape
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(B, Cc, T, device=x.device, dtype=out_dtype or x.dtype)
    _chk(out, 'out', _F32_OR_BF16)
    check(lib.ag_transpose_batched(_p(x), int(_is16(x)), Cc, B * Cc, _p(out), int(_is16(out)), Cc * T, T, B, T, Cc, _stream()),
          'ag_transpose_batched')
    return out


def rowdot_ok(x, w):
    """can the one-output Linear kernels (ag_rowdot_*) take x [M,K] (unit stride along K) and w [1,K] / [K]?"""
    return x.dim() == 2 and x.stride(1) == 1 and w.numel() == x.size(1) and w.is_contiguous()


@_timed()
def rowdot_fwd(x, w, bias, y):
    """y[m] = x[m,:] . w + bias[0]; y: [M] or [M,1] of any stride; x fp32 or bf16"""
    ldx = _mat(x, 'x', _F32_OR_BF16)
    _chk(w, 'w'); _chk(bias, 'bias'); _chk(y, 'y')
    M, Kd = x.shape
    assert rowdot_ok(x, w) and y.numel() == M
    ldy = y.stride(0) if M > 1 else 1
    check(lib.ag_rowdot_fwd(_p(x), int(_is16(x)), ldx, _p(w), _p(bias), _p(y), ldy, M, Kd, _stream()), 'ag_rowdot_fwd')


@_timed()
def rowdot_bwd(dy, x, w, dx=None, dw=None, db=None, gate=False, slope=LEAKY_SLOPE, accumulate=True):
    """backward of a one-output Linear in ONE pass over x: dx = dy (x) w (times LeakyReLU'(x) when ``gate``: x is the saved
    output of the LeakyReLU below), dw (+)= dy^T x, db (+)= sum dy.  dw [1,K] / [K] and db [1] must be adjacent in memory
    (db right behind dw: one gradient row), as the views of WNGroup.zero_dws are; dy: [M] or [M,1] of any stride."""
    ldx = _mat(x, 'x', _F32_OR_BF16)
    _chk(dy, 'dy'); _chk(w, 'w'); _chk(dx, 'dx', _F32_OR_BF16); _chk(dw, 'dw'); _chk(db, 'db')
    M, Kd = x.shape
    assert rowdot_ok(x, w) and dy.numel() == M
    lddx = _mat(dx, 'dx', _F32_OR_BF16) if dx is not None else 0
    assert dx is None or (tuple(dx.shape) == (M, Kd) and dx.dtype == x.dtype), 'x and dx share a storage type'
    h16 = int(_is16(x))
    if dw is not None:
        assert dw.is_contiguous() and dw.numel() == Kd and db is not None and db.numel() == 1
        assert db.data_ptr() == dw.data_ptr() + 4 * Kd, 'db must sit right behind dw'
        _ws = _bind_ws(lib.ag_rowdot_bwd_ws_numel(M, Kd), dw.device)  # noqa: F841
    check(lib.ag_rowdot_bwd(_p(dy), dy.stride(0) if M > 1 else 1, _p(x), ldx, _p(w), _p(dx), lddx, h16, _p(dw), _p(db),
                            int(bool(accumulate)), M, Kd, int(bool(gate)), slope, _stream()), 'ag_rowdot_bwd')


@_timed()
def to_bf16(src, out=None):
    """a bfloat16 image of a contiguous or row-pitched 2-D fp32 tensor / of any contiguous fp32 tensor (ag_to_bf16_2d)"""
    _chk(src, 'src')
    if src.dim() == 2 and src.stride(1) == 1 and src.size(0) <= 65535:
        rows, cols, ld = src.size(0), src.size(1), (src.stride(0) if src.size(0) > 1 else src.size(1))
    else:
        assert src.is_contiguous()
        n = src.numel()
        cols = next((c for c in (8192, 4096, 2048, 1024, 512, 256, 64, 8, 1) if n % c == 0 and n // c <= 65535), None)
        assert cols is not None, 'to_bf16: tensor too large for one launch'
        rows, ld = n // cols, cols
    if out is None:
        out = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
    _chk(out, 'out', torch.bfloat16)
    assert out.is_contiguous() and out.numel() == src.numel()
    check(lib.ag_to_bf16_2d(_p(src), ld, _p(out), cols, rows, cols, _stream()), 'ag_to_bf16_2d')
    return out


def gemm_h_ok(A, B, ta, tb):
    """can ag_gemm_h take these bf16 operands?  (K % 64 == 0, 16-byte aligned rows, k-strided row counts % 8 == 0)"""
    if not (_is16(A) and _is16(B) and A.dim() == 2 and B.dim() == 2 and A.stride(1) == 1 and B.stride(1) == 1):
        return False
    M, Kd = (A.size(1), A.size(0)) if ta else (A.size(0), A.size(1))
    N = B.size(0) if tb else B.size(1)
    lda = A.stride(0) if A.size(0) > 1 else A.size(1)
    ldb = B.stride(0) if B.size(0) > 1 else B.size(1)
    return bool(lib.ag_gemm_h_ok(M, N, Kd, int(ta), int(tb), lda, ldb)) and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0


def _work_gemm_h(A, B, C=None, C16=None, ta=False, tb=False, *a_, **kw):
    out = C if C is not None else C16
    M, N = out.shape
    Kd = A.size(0) if ta else A.size(1)
    return None, 2.0 * M * N * Kd, 2.0 * (M * Kd + N * Kd) + (4.0 if C is not None else 2.0) * M * N


@_timed(_work_gemm_h)
def gemm_h(A, B, C=None, C16=None, ta=False, tb=False, alpha=1.0, beta=0.0, bias=None, res=None, gate=None, act=ACT_NONE,
           slope=LEAKY_SLOPE, defer=False):
    """C / C16 [M,N] = act(alpha * op(A) @ op(B) + beta * C + bias + res) on operands STORED as bfloat16 (ag_gemm_h).
    C: fp32 output, C16: bf16 output (either or both); res: fp32 or bf16 residual (with ACT_LEAKY_GATE: the saved activation);
    gate: bf16 saved LeakyReLU output applied after bias / res.  ``defer`` as for gemm()."""
    lda, ldb = _mat(A, 'A', _F32_OR_BF16), _mat(B, 'B', _F32_OR_BF16)
    assert _is16(A) and _is16(B), 'gemm_h: bf16 operands'
    out = C if C is not None else C16
    M, N = out.shape
    Kd = A.size(0) if ta else A.size(1)
    assert (A.size(1) if ta else A.size(0)) == M, 'gemm_h: A shape'
    assert (B.size(1) if tb else B.size(0)) == Kd and (B.size(0) if tb else B.size(1)) == N, 'gemm_h: B shape'
    ldc = ldc16 = ldres = ldres16 = ldg = 0
    if C is not None:
        ldc = _mat(C, 'C')
        assert tuple(C.shape) == (M, N)
    if C16 is not None:
        _chk(C16, 'C16', torch.bfloat16)
        ldc16 = _mat(C16, 'C16', _F32_OR_BF16)
        assert tuple(C16.shape) == (M, N)
    r32 = res if (res is not None and not _is16(res)) else None
    r16 = res if _is16(res) else None
    if res is not None:
        assert tuple(res.shape) == (M, N)
        ldres, ldres16 = (_mat(r32, 'res') if r32 is not None else 0), (_mat(r16, 'res', _F32_OR_BF16) if r16 is not None else 0)
    if gate is not None:
        _chk(gate, 'gate', torch.bfloat16)
        ldg = _mat(gate, 'gate', _F32_OR_BF16)
        assert tuple(gate.shape) == (M, N)
    if bias is not None:
        _chk(bias, 'bias')
        assert bias.numel() == N and bias.is_contiguous()
    nws = lib.ag_gemm_h_ws_numel(M, N, Kd, act, int(C16 is not None)) if gate is None else 0
    hold = (not defer) and nws > 0 and reduces_recording()
    if hold:
        lib.ag_defer_reduces(2)
    try:
        _ws = _bind_ws(nws, out.device)  # noqa: F841
        check(lib.ag_gemm_h(_p(A), lda, int(ta), _p(B), ldb, int(tb), _p(C), ldc, _p(C16), ldc16, M, N, Kd, alpha, beta,
                            _p(bias), _p(r32), ldres, _p(r16), ldres16, _p(gate), ldg, act, slope, _stream()), 'ag_gemm_h')
    finally:
        if hold:
            lib.ag_defer_reduces(3)


@_timed()
def build_zc(z, c, out=None):
    """zc[t,b,:] = [z[b,t,:] | c[b,:]]: z [B,T,ns], c [B,es] -> contiguous [T,B,ns+es] (ag_build_zc; audiogan.py:433-439)"""
    _chk(z, 'z'); _chk(c, 'c')
    B, T, ns = z.shape
    es = c.size(1)
    assert z.is_contiguous() and c.is_contiguous() and c.size(0) == B
    if out is None:
        out = torch.empty(T, B, ns + es, device=z.device)
    check(lib.ag_build_zc(_p(z), _p(c), _p(out), B, T, ns, es, _stream()), 'ag_build_zc')
    return out


@_timed()
def critic_batch(xa, na=None, xb=None, nb=None, len_a=None, len_b=None, prods=(), ca=None, cb=None):
    """the critic's minibatch in ONE launch (ag_critic_batch): rows [xa + na ; xb + nb] -> x [nA+nB, L]; the rows' lengths
    after every conv layer, lens [len(prods), nA+nB] int64 with lens[i] = ceil(len / prods[i]) (len_a / len_b None: L); the
    conditioning rows [ca ; cb] (None: skipped).  Returns (x, lens or None, c or None)."""
    nA, L = xa.shape
    nB = xb.size(0) if xb is not None else 0
    dev = xa.device
    lda = _rows(xa, 'xa', nA, L)
    ldna = _rows(na, 'na', nA, L) if na is not None else 0
    ldb = _rows(xb, 'xb', nB, L) if xb is not None else 0
    ldnb = _rows(nb, 'nb', nB, L) if nb is not None else 0
    for t_, n_, k_ in ((len_a, 'len_a', nA), (len_b, 'len_b', nB)):
        _chk(t_, n_, torch.int64)
        assert t_ is None or (t_.is_contiguous() and t_.numel() == k_)
    x = torch.empty(nA + nB, L, device=dev)
    nl = len(prods)
    lens = torch.empty(nl, nA + nB, dtype=torch.int64, device=dev) if nl else None
    E, c = 0, None
    if ca is not None:
        E = ca.size(1)
        for t_, n_, k_ in ((ca, 'ca', nA), (cb, 'cb', nB)):
            _chk(t_, n_)
            assert t_ is None or (t_.is_contiguous() and tuple(t_.shape) == (k_, E))
        assert cb is not None or nB == 0
        c = torch.empty(nA + nB, E, device=dev)
    arr = (C.c_int32 * max(nl, 1))(*[int(v) for v in prods])
    check(lib.ag_critic_batch(_p(xa), lda, _p(na), ldna, nA, _p(xb), ldb, _p(nb), ldnb, nB, L, _p(x), _p(len_a), _p(len_b),
                              arr, nl, _p(lens), _p(ca), _p(cb), E, _p(c), _stream()), 'ag_critic_batch')
    return x, lens, c


@_timed()
def axpby(x, y, a, b):
    """y = a*x + b*y (contiguous)"""
    _chk(x, 'x'); _chk(y, 'y')
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    check(lib.ag_axpby(_p(x), _p(y), x.numel(), float(a), float(b), _stream()), 'ag_axpby')


# ------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------
def _opt_table(params, grads, s1, s2):
    descs = []
    for i, p in enumerate(params):
        _chk(p, 'param'); _chk(grads[i], 'grad'); _chk(s1[i], 's1')
        assert p.is_contiguous() and grads[i].is_contiguous() and grads[i].numel() == p.numel()
        descs.append(_lib.OptDesc(p.data_ptr(), grads[i].data_ptr(), s1[i].data_ptr(),
                                  s2[i].data_ptr() if s2 is not None else 0, p.numel()))
    return _table('opt', descs, params[0].device)


@_timed()
def grad_norms(params, grads, s1, s2, norms, norm_sum, flags, grad_scale=1.0, step_dev=None, finish=True):
    """norms[i] = ||grads[i]*grad_scale||; norm_sum[0] = sum_i norms[i]; flags = NaN/BIG bits (written).  ``finish=False``:
    only the per-chunk partial sums are computed; returns the workspace holding them, to be handed to ``opt_step(part=...)``
    right behind on the same stream (norms / norm_sum / flags are then written by that launch)."""
    tab = _opt_table(params, grads, s1, s2)
    _chk(norms, 'norms'); _chk(norm_sum, 'norm_sum'); _chk(flags, 'flags', torch.int32)
    assert norms.numel() >= len(params)
    _chk(step_dev, 'step_dev', torch.int32)
    ws = torch.empty(512 * len(params), dtype=torch.float32, device=norms.device)
    check(lib.ag_bind_workspace(_p(ws), ws.numel()), 'ag_bind_workspace')
    check(lib.ag_grad_norms(_p(tab), len(params), _p(norms), _p(norm_sum), _p(flags), grad_scale,
                            _p(step_dev), int(bool(finish)), _stream()), 'ag_grad_norms')
    return ws


@_timed()
def opt_step(params, grads, s1, s2, norms, kind, lr, clip, grad_scale, a1, b2, eps, step, step_dev=None, part=None,
             norm_sum=None, flags=None):
    """``part``: the workspace ``grad_norms(finish=False)`` returned - this launch then also finishes the norms"""
    tab = _opt_table(params, grads, s1, s2)
    _chk(step_dev, 'step_dev', torch.int32); _chk(part, 'part'); _chk(norm_sum, 'norm_sum'); _chk(flags, 'flags', torch.int32)
    assert part is None or part.numel() >= 512 * len(params)
    check(lib.ag_opt_step(_p(tab), len(params), _p(norms), kind, lr, clip, grad_scale, a1, b2, eps,
                          step, _p(step_dev), _p(part), _p(norms) if part is not None else None, _p(norm_sum), _p(flags),
                          _stream()), 'ag_opt_step')


# ------------------------------------------------------------------------------------
# exponential moving average of a parameter list (optim.EMA)
# ------------------------------------------------------------------------------------
EMA_CHUNK = int(lib.ag_ema_chunk())
_ema_plans = OrderedDict()       # (shadow ptr, param ptr, numel) per tensor -> plan


def ema_plan(shadows, params):
    """-> (bytes, chunks, tensors): the checked descriptors followed by the chunk-to-tensor map ([chunks][2] int32: tensor,
    chunk inside it), built once per list of tensors.  The bytes go through ``_table`` on every ``ema_update``, so the
    device copy is cached / pinned under capture exactly as the optimiser's table is.  A caller that keeps its tensors
    (optim.EMA) may keep the plan and hand it back: the per-tensor checks then run once, not per launch."""
    assert len(shadows) == len(params) and len(params) > 0
    for e, p in zip(shadows, params):
        _chk(e, 'shadow'); _chk(p, 'param')
        assert e.is_contiguous() and p.is_contiguous() and e.numel() == p.numel() >= 1, (tuple(e.shape), tuple(p.shape))
        assert e.device == p.device == params[0].device
    sig = tuple((e.data_ptr(), p.data_ptr(), p.numel()) for e, p in zip(shadows, params))
    plan = _ema_plans.get(sig)
    if plan is not None:
        _ema_plans.move_to_end(sig)
        return plan
    descs = [_lib.EmaDesc(*t) for t in sig]
    counts = np.asarray([(t[2] + EMA_CHUNK - 1) // EMA_CHUNK for t in sig], dtype=np.int64)
    total = int(counts.sum())
    assert total < 2 ** 31
    cmap = np.empty((total, 2), dtype=np.int32)
    cmap[:, 0] = np.repeat(np.arange(len(counts)), counts)
    cmap[:, 1] = np.arange(total) - np.repeat(np.cumsum(counts) - counts, counts)
    plan = (b''.join(bytes(d) for d in descs) + cmap.tobytes(), total, len(sig))
    _ema_plans[sig] = plan
    while len(_ema_plans) > 64:
        _ema_plans.popitem(last=False)
    return plan


def _work_ema(shadows, params, *a_, **kw):
    return 'ema_update_kernel', 0.0, 12.0 * sum(p.numel() for p in params)


@_timed(_work_ema)
def ema_update(shadows, params, decay, warmup, step_dev, step0, k=0, plan=None):
    """shadows[i] = lerp(shadows[i], params[i], 1 - d) for the whole list in ONE launch (ag_ema_update): per element
    ``e = fmaf(1 - d, p - e, e)`` in fp32; d = decay, or with ``warmup`` min(decay, (1 + k) / (10 + k)) where
    k = max(0, step_dev[0] - step0) (``step_dev``: the optimiser's int32 device step counter, only read) or the host ``k``
    when ``step_dev`` is None.  Tensors: fp32, contiguous, any numel >= 1, any 4-byte alignment; ``params`` are not
    written.  ``plan``: what ``ema_plan(shadows, params)`` returned for these very tensors."""
    decay = float(decay)
    if not 0.0 <= decay <= 1.0:
        raise ValueError('audiogan_amd: ema_update needs 0 <= decay <= 1, got %r' % (decay,))
    _chk(step_dev, 'step_dev', torch.int32)
    raw, chunks, n = plan if plan is not None else ema_plan(shadows, params)
    assert n == len(params) == len(shadows)
    tab = _table('ema', [raw], params[0].device)
    check(lib.ag_ema_update(_p(tab), n, C.c_void_p(tab.data_ptr() + n * C.sizeof(_lib.EmaDesc)), chunks, decay,
                            int(bool(warmup)), _p(step_dev), int(step0), int(k), _stream()), 'ag_ema_update')


# ------------------------------------------------------------------------------------
# skinny products / fused recurrent steps (lstm_step.hip)
# ------------------------------------------------------------------------------------
def _al16(t):
    return t.data_ptr() % 16 == 0


def skinny_ok(A, B, tb):
    """can ag_skinny_gemm take this product? (M <= 256, K % 8 == 0, 16-byte aligned rows)"""
    M, Kd = A.shape
    ok = M <= 256 and Kd % 8 == 0 and A.stride(1) == 1 and A.stride(0) % 4 == 0 and _al16(A)
    if tb:
        ok = ok and B.stride(1) == 1 and B.stride(0) % 4 == 0 and _al16(B)
    return ok


def _work_skinny(A, B, Cm, tb=False, *a_, **kw):
    M, N = Cm.shape
    return 'skinny_gemm_kernel', 2.0 * M * N * A.size(1), \
        4.0 * (A.numel() + N * A.size(1) + M * N)


@_timed(_work_skinny)
def skinny_gemm(A, B, Cm, tb=False, beta=0.0, bias=None, act=ACT_NONE, slope=LEAKY_SLOPE, atomic=False):
    """Cm[M<=256,N] = act(A @ op(B) + beta*Cm + bias), or with atomic=True: Cm += A @ op(B) (+bias).  ``atomic`` means
    "accumulate through the two-stage workspace" (bound here, summed in a fixed order); no atomic instruction is involved"""
    lda, ldb, ldc = _mat(A, 'A'), _mat(B, 'B'), _mat(Cm, 'C')
    M, N = Cm.shape
    Kd = A.size(1)
    assert A.size(0) == M and (B.size(1) if tb else B.size(0)) == Kd and (B.size(0) if tb else B.size(1)) == N
    if bias is not None:
        _chk(bias, 'bias')
        assert bias.numel() == N and bias.is_contiguous()
    _ws = _bind_ws(lib.ag_skinny_ws_numel(M, N, Kd), Cm.device) if atomic else None  # noqa: F841
    check(lib.ag_skinny_gemm(_p(A), lda, _p(B), ldb, int(tb), _p(Cm), ldc, M, N, Kd, beta, _p(bias), act,
                             slope, int(atomic), _stream()), 'ag_skinny_gemm')


def lstm_front_bwd_ok(B, H, fs, dxa_t, x_t):
    return (H % 16 == 0 and fs % 16 == 0 and B <= 65535 and dxa_t.stride(1) == 1 and x_t.stride(1) == 1
            and dxa_t.stride(0) % 4 == 0 and x_t.stride(0) % 4 == 0 and _al16(dxa_t) and _al16(x_t))


def lstm_front_bwd_step(dxa_t, x_t, gx_out, w_proj, dh_acc, gates, c_prev, c_new, dc_next, dgates, dc_prev):
    """fused backward of one Generator-front frame: gx = dxa_t*(1-x_t^2) -> gx_out; dh = dh_acc + gx @ w_proj;
    LSTMCell backward -> dgates, dc_prev.  dxa_t / x_t: [B,fs] row views; the rest contiguous."""
    B, fs = dxa_t.shape
    H = w_proj.size(1)
    for t_, n, shp in ((gx_out, 'gx_out', (B, fs)), (w_proj, 'w_proj', (fs, H)),
                       (gates, 'gates', (B, 4 * H)), (c_prev, 'c_prev', (B, H)), (c_new, 'c_new', (B, H)),
                       (dgates, 'dgates', (B, 4 * H)), (dc_prev, 'dc_prev', (B, H))):
        _chk(t_, n)
        assert t_.is_contiguous() and tuple(t_.shape) == shp, (n, tuple(t_.shape), shp)
    _chk(dxa_t, 'dxa_t'); _chk(x_t, 'x_t'); _chk(dc_next, 'dc_next'); _chk(dh_acc, 'dh_acc')
    assert tuple(x_t.shape) == (B, fs) and lstm_front_bwd_ok(B, H, fs, dxa_t, x_t)
    assert tuple(dh_acc.shape) == (B, H) and dh_acc.stride(1) == 1
    assert dc_next is None or (dc_next.is_contiguous() and tuple(dc_next.shape) == (B, H))
    check(lib.ag_lstm_front_bwd_step(_p(dxa_t), dxa_t.stride(0), _p(x_t), x_t.stride(0), _p(gx_out), fs, fs,
                                     _p(w_proj), _p(dh_acc), dh_acc.stride(0), _p(gates), _p(c_prev), _p(c_new), _p(dc_next),
                                     _p(dgates), _p(dc_prev), B, H, _stream()), 'ag_lstm_front_bwd_step')


def lstm_step_ok(B, H, x=None, wx=None):
    ok = B <= 256 and H % 8 == 0
    if x is not None:
        ok = ok and x.size(1) % 8 == 0 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and _al16(x) \
            and wx.stride(1) == 1 and wx.stride(0) % 4 == 0 and _al16(wx)
    return ok


def _work_step(gates_pre, x, wx, h_prev, whh, *a_, **kw):
    B, H4 = gates_pre.shape
    Kd = H4 // 4 + (x.size(1) if x is not None else 0)
    return 'lstm_step_fwd_kernel', 2.0 * B * H4 * Kd, 4.0 * (H4 * Kd + 3 * B * H4)


@_timed(_work_step)
def lstm_step_fwd(gates_pre, x, wx, h_prev, whh, c_prev, c_out, h_out, first_step):
    """fused LSTMCell step; gates_pre [B,4H] contiguous is overwritten with the activated gates"""
    for t_, n in ((gates_pre, 'gates_pre'), (h_prev, 'h_prev'), (whh, 'whh'), (c_prev, 'c_prev'),
                  (c_out, 'c_out'), (h_out, 'h_out')):
        _chk(t_, n)
        assert t_.is_contiguous()
    B, H4 = gates_pre.shape
    H = H4 // 4
    ldx = ldwx = Kx = 0
    if x is not None:
        ldx, ldwx, Kx = _mat(x, 'x'), _mat(wx, 'wx'), x.size(1)
        assert wx.size(0) == 4 * H and wx.size(1) == Kx
    check(lib.ag_lstm_step_fwd(_p(gates_pre), _p(x), ldx, _p(wx), ldwx, Kx, _p(h_prev), _p(whh), _p(c_prev),
                               _p(c_out), _p(h_out), B, H, int(first_step), _stream()), 'ag_lstm_step_fwd')


def _ptr_table(tensors):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def _rows(t, name, B, n):
    """row pitch of a [B, n] view with unit stride along dim 1 (a slab channel, a column block)"""
    _chk(t, name)
    assert t.dim() == 2 and tuple(t.shape) == (B, n) and (n == 1 or t.stride(1) == 1), (name, tuple(t.shape), t.stride())
    return t.stride(0) if B > 1 else max(t.stride(0), n)


_PITCHED = 'pitched'      # mark in a _check_table row: a 2-D view of unit stride along dim 1 and any row pitch


def _check_table(table):
    """the tensor checks of the recurrent launches.  Rows (tensor, name, shape[, kind]): a device tensor of that shape and of
    the dtype ``kind`` (fp32 by default; _F32_OR_BF16: either), dense unless ``kind`` is _PITCHED (fp32; channel 0 of a slab,
    a column block of a weight).  A tensor that is None (an optional one) is skipped.  Returns {name: row pitch} of the
    _PITCHED rows (0: None)"""
    ld = {}
    for t, name, shp, *kind in table:
        if kind == [_PITCHED]:
            ld[name] = _rows(t, name, *shp) if t is not None else 0
        elif t is not None:
            _chk(t, name, *kind)
            assert t.is_contiguous() and tuple(t.shape) == shp, (name, tuple(t.shape), shp)
    return ld


def _per_dir(ndir, *lists):
    """_check_table rows of an LSTM layer pass: (list, name, shape[, kind]), a list of one tensor per direction or None (an
    optional list), gives one row per direction, named name[d]"""
    rows = []
    for lst, name, *rest in lists:
        if lst is not None:
            assert len(lst) == ndir, (name, len(lst), ndir)
            rows += [(t, '%s[%d]' % (name, d)) + tuple(rest) for d, t in enumerate(lst)]
    return rows


# ---- persistent (weights-resident) layer pass: workspace per device, status word, switch -------------------------
PERSIST = [os.environ.get('AG_LSTM_PERSIST', '1') != '0']
_persist_ws = {}
_ncu = {}


def _n_cu(dev):
    n = _ncu.get(dev)
    if n is None:
        n = _ncu[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return n


def _persist_ok(rule, dims, dev, on=True):
    """the one rule by which a persistent launch is offered: PERSIST[0] and the launch's own switches (``on``), a CUDA device,
    and the library's shape rule for the device's CU count, lib.<rule>(*dims, n_cu)"""
    return bool(PERSIST[0] and on and torch.device(dev).type == 'cuda' and rule(*dims, _n_cu(dev)))


def lstm_persist_ok(B, H, ndir, dev):
    return _persist_ok(lib.ag_lstm_persist_ok, (B, H, ndir), dev)


_PERSIST_WS_MIN = 8 << 20      # covers every BASELINE shape (biLSTM at 256 clips, H 768: 3.2 MB; the generator front: 0.7 MB)


def _persist_workspace(dev, nbytes):
    """the per-device workspace of the persistent launches (sticky status word + header + exchange buffers).  Allocated
    once at a size that covers every shape the kernels accept at BASELINE batch sizes; if a later call still needs more,
    a NEW buffer becomes current and the old one stays alive for good: a captured hipGraph has its pointer baked into
    memset and kernel nodes and keeps using it on every replay (freeing it would hand that memory to another tensor)."""
    lst = _persist_ws.setdefault(dev, [])
    if not lst or lst[0].numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('audiogan_amd: the persistent LSTM workspace must exist before hipGraph capture '
                               '(run one eager step first)')
        lst.insert(0, torch.zeros(max(int(nbytes), _PERSIST_WS_MIN), dtype=torch.uint8, device=dev))
    return lst[0]


def lstm_persist_status(dev=None, reset=False):
    """sticky status of EVERY persistent launch on `dev` since the workspace was allocated (or since the last
    ``reset=True``): 0 = all completed (host sync).  Non-zero: a bounded wait timed out, i.e. a launch's workgroups were
    not all co-resident (another persistent or RCCL kernel holding CUs, a CU mask, a partition mode); everything that
    launch produced afterwards is NaN."""
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else torch.device(dev)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    st = 0
    for ws in _persist_ws.get(dev, []):
        st |= int(ws[:4].view(torch.int32).item()) & 0xFFFFFFFF
        if reset:
            ws[:4].zero_()
    return st


class PersistentLaunchError(RuntimeError):
    pass


def check_persist_status(dev=None):
    """raise if any persistent launch on `dev` gave up (see lstm_persist_status); resets the sticky word"""
    st = lstm_persist_status(dev)
    if st:
        lstm_persist_status(dev, reset=True)
        raise PersistentLaunchError(persist_error_text(st))


def persist_error_text(st):
    """what ``check_persist_status`` says about a non-zero sticky word (summary.Summary.drain raises the same)"""
    return ('audiogan_amd: a persistent recurrent launch timed out waiting for its group (status 0x%08x: step %d); its '
            'workgroups were not all co-resident - is another persistent or collective kernel holding compute units? '
            'Results of that launch are NaN.  AG_LSTM_PERSIST=0 selects the per-step kernels.' % (st, st & 0x7FFFFFFF))


def persist_debug(timeout_ticks=0, mute_block=-1):
    """test hook (ag_persist_debug)"""
    check(lib.ag_persist_debug(int(timeout_ticks), int(mute_block)), 'ag_persist_debug')


def lstm_seq_fwd_persist(pre, whh, c_all, y, valid, static=None):
    """ONE persistent launch for the whole layer pass (ag_lstm_seq_fwd_persist)"""
    ndir = len(pre)
    T, B, H4 = pre[0].shape
    H = H4 // 4
    _check_table(_per_dir(ndir, (pre, 'pre', (T, B, 4 * H)), (whh, 'whh', (4 * H, H)), (c_all, 'c_all', (T + 1, B, H)),
                          (static, 'static', (B, 4 * H))) + [(y, 'y', (T, B, ndir * H), _F32_OR_BF16)])
    _chk(valid, 'valid', torch.int64)
    nb = int(lib.ag_lstm_persist_ws_bytes(B, H, ndir))
    ws = _persist_workspace(y.device, nb)
    check(lib.ag_lstm_seq_fwd_persist(_ptr_table(pre), _ptr_table(whh), _ptr_table(c_all), _p(y), int(_is16(y)), _p(valid),
                                      _ptr_table(static) if static is not None else None, _p(ws), ws.numel(),
                                      T, B, H, ndir, _n_cu(y.device), _stream()), 'ag_lstm_seq_fwd_persist')


def _work_seq_fwd_persist(pre, whh, c_all, y, valid, static=None):
    T, B, H4 = pre[0].shape
    nd = len(pre)
    # one launch = the whole layer pass: T steps of 2*B*4H*H flops per direction; algorithmic bytes: W_hh ONCE
    # + gates in/out, cells, outputs per step
    return 'lstm_persist_fwd_kernel' + _bf16_tag(), T * 2.0 * nd * B * H4 * (H4 // 4), \
        4.0 * nd * (H4 * (H4 // 4) + T * 3 * B * H4), 1


# (the public wrapper stays untimed: lstm_seq_fwd goes through this name)
_lstm_seq_fwd_persist_call = _timed(_work_seq_fwd_persist, name='_lstm_seq_fwd_persist_call')(lstm_seq_fwd_persist)


def lstm_seq_fwd(pre, whh, c_all, hbuf, y, valid, static=None):
    """pre/whh/c_all/hbuf: lists (one per direction) of contiguous tensors; static: optional list of [B,4H]
    tensors added to every step's pre-activations; see ag_lstm_seq_fwd.  Shapes that fit the chip take the
    persistent weights-resident launch (AG_LSTM_PERSIST=0 forces one launch per step)."""
    T = pre[0].size(0)
    if lstm_persist_ok(pre[0].size(1), pre[0].size(2) // 4, len(pre), y.device):
        _lstm_seq_fwd_persist_call(pre, whh, c_all, y, valid, static)
        return
    # (the profiler times the whole chain of T back-to-back launches with one pair of events and divides by T:
    # events around every single launch add ~3 us to a 10 us kernel)
    _lstm_seq_fwd_range(pre, whh, c_all, hbuf, y, valid, 0, T, static)


def _work_seq_fwd(pre, whh, c_all, hbuf, y, valid, k0, k1, *a_, **kw):
    T, B, H4 = pre[0].shape
    nd, n = len(pre), k1 - k0
    return 'lstm_step_fwd_kernel', n * 2.0 * nd * B * H4 * (H4 // 4), n * 4.0 * nd * (H4 * (H4 // 4) + 3 * B * H4), n


@_timed(_work_seq_fwd)
def _lstm_seq_fwd_range(pre, whh, c_all, hbuf, y, valid, k0, k1, static=None):
    ndir = len(pre)
    T, B, H4 = pre[0].shape
    H = H4 // 4
    _check_table(_per_dir(ndir, (pre, 'pre', (T, B, 4 * H)), (whh, 'whh', (4 * H, H)), (c_all, 'c_all', (T + 1, B, H)),
                          (hbuf, 'hbuf', (2, B, H)), (static, 'static', (B, 4 * H))) + [(y, 'y', (T, B, ndir * H))])
    _chk(valid, 'valid', torch.int64)
    check(lib.ag_lstm_seq_fwd(_ptr_table(pre), _ptr_table(whh), _ptr_table(c_all), _ptr_table(hbuf), _p(y),
                              _p(valid), _ptr_table(static) if static is not None else None, T, B, H, ndir, k0, k1,
                              _stream()), 'ag_lstm_seq_fwd')


def gfront_persist_ok(B, S, fs, dev):
    return _persist_ok(lib.ag_gfront_persist_ok, (B, S, fs), dev)


def _front_launch(entry, args, dev, ws_bytes):
    """fills in what every launch of the fronts sets the same way (struct size, workspace, CUs) and calls lib.<entry>"""
    ws = _persist_workspace(dev, ws_bytes)
    args.struct_bytes, args.ws, args.ws_bytes, args.n_cu = C.sizeof(args), ws.data_ptr(), ws.numel(), _n_cu(dev)
    check(getattr(lib, entry)(C.byref(args), _stream()), entry)


def _work_gfront(gates, wx, whh, wp, *a_, **kw):
    T, B, S4 = gates.shape
    S, fs = S4 // 4, wp.size(0)
    return 'gfront_persist_fwd_kernel' + _bf16_tag(), T * 2.0 * B * (S4 * (S + fs) + fs * S), \
        4.0 * (S4 * (S + fs) + fs * S + T * B * (2 * S4 + 2 * S + fs)), 1


@_timed(_work_gfront)
def gfront_fwd_persist(gates, wx, whh, wp, bp, hs, cs, x, xt=None):
    """the Generator front's frame loop in ONE persistent launch (ag_gfront_fwd, LSTM cell, training).  x: [B, T*fs] rows of
    any pitch (channel 0 of the conv trunk's slab); xt: optional [T,B,fs], receives the same frames time-major"""
    T, B, S4 = gates.shape
    S = S4 // 4
    fs = wp.size(0)
    ld = _check_table(((gates, 'gates', (T, B, 4 * S)), (whh, 'whh', (4 * S, S)), (wp, 'wp', (fs, S)), (bp, 'bp', (fs,)),
                       (hs, 'hs', (T, B, S)), (cs, 'cs', (T + 1, B, S)), (xt, 'xt', (T, B, fs)),
                       (x, 'x', (B, T * fs), _PITCHED), (wx, 'wx', (4 * S, fs), _PITCHED)))
    a = _lib.FrontFwdArgs(cell=0, gen=0, gates=_p(gates), w_x=_p(wx), ldwx=ld['wx'], w_hh=_p(whh), w_p=_p(wp), b_p=_p(bp),
                          hs=_p(hs), cs=_p(cs), x=_p(x), ldx=ld['x'], xt=_p(xt), T=T, B=B, S=S, fs=fs)
    _front_launch('ag_gfront_fwd', a, x.device, int(lib.ag_gfront_persist_ws_bytes(B, S, fs)))


# the front's backward runs beside the conv trunk's gradient all-reduce in the multi-GPU step (train.GraphedStep, phase
# g3b; eager: the bucket's hook): a persistent launch wants its CUs to itself, so a generator whose optimiser carries a
# gradient bucket runs its backward with this switch off (train.g_step / g_backward / GraphedStep)
PERSIST_FRONT_BWD = [True]


class front_bwd_persist(object):
    """``with K.front_bwd_persist(on): loss.backward()`` - `on` False: the front's backward takes the per-frame form"""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.old = PERSIST_FRONT_BWD[0]
        PERSIST_FRONT_BWD[0] = self.old and self.on

    def __exit__(self, *exc):
        PERSIST_FRONT_BWD[0] = self.old


def gfront_bwd_persist_ok(B, S, fs, dev):
    return _persist_ok(lib.ag_gfront_bwd_persist_ok, (B, S, fs), dev, PERSIST_FRONT_BWD[0])


def _work_gfront_bwd(gates, cs, x, dh_ext, dx_ext, whh, wx, wp, *a_, **kw):
    T, B, S4 = gates.shape
    S, fs = S4 // 4, wp.size(0)
    return 'gfront_persist_bwd_kernel' + _bf16_tag(), 2.0 * B * ((T - 1) * S4 * (S + fs) + T * fs * S), \
        4.0 * (S4 * (S + fs) + fs * S + T * B * (2 * S4 + 2 * S + (S + fs) + 2 * fs)), 1


@_timed(_work_gfront_bwd)
def gfront_bwd_persist(gates, cs, x, dh_ext, dx_ext, whh, wx, wp, dgs, dxt):
    """the backward through time of the Generator front's frame loop in ONE persistent launch (ag_gfront_bwd, LSTM cell);
    the external gradients, read only, each may be None: dh_ext [T,B,S] = dL/dh_t (the stop head's), dx_ext [B,T*fs] rows of
    any pitch = dL/dx_t (the conv trunk's: channel 0 of its gradient slab); x likewise [B,T*fs] rows of any pitch"""
    T, B, S4 = gates.shape
    S = S4 // 4
    fs = wp.size(0)
    ld = _check_table(((gates, 'gates', (T, B, 4 * S)), (cs, 'cs', (T + 1, B, S)), (whh, 'whh', (4 * S, S)),
                       (wp, 'wp', (fs, S)), (dgs, 'dgs', (T, B, 4 * S)), (dxt, 'dxt', (T, B, fs)), (dh_ext, 'dh_ext', (T, B, S)),
                       (x, 'x', (B, T * fs), _PITCHED), (dx_ext, 'dx_ext', (B, T * fs), _PITCHED),
                       (wx, 'wx', (4 * S, fs), _PITCHED)))
    a = _lib.FrontBwdArgs(cell=0, ga=_p(gates), state=_p(cs), x=_p(x), ldx=ld['x'], dh_ext=_p(dh_ext), dx_ext=_p(dx_ext),
                          lddx=ld['dx_ext'], w_hh=_p(whh), w_x=_p(wx), ldwx=ld['wx'], w_p=_p(wp), dgs=_p(dgs), dxt=_p(dxt),
                          T=T, B=B, S=S, fs=fs)
    _front_launch('ag_gfront_bwd', a, x.device, _PERSIST_WS_MIN)


def _work_grufront_bwd(gates, hs, gh, x, dh_ext, dx_ext, whh, wx, wp, *a_, **kw):
    T, B, S3 = gates.shape
    S, fs = S3 // 3, wp.size(0)
    return 'gfront_persist_bwd_kernel<gru>', 2.0 * B * ((T - 1) * S3 * (S + fs) + T * fs * S), \
        4.0 * (S3 * (S + fs) + fs * S + T * B * (4 * S3 + 2 * S + (S + fs) + 2 * fs)), 1


@_timed(_work_grufront_bwd)
def grufront_bwd_persist(gates, hs, gh, x, dh_ext, dx_ext, whh, wx, wp, dgi, dgh, dxt):
    """the GRU front's backward through time in ONE persistent launch (ag_gfront_bwd, GRU cell); hs [T+1,B,S] with
    hs[t] = h_{t-1}; dh_ext / dx_ext: the external gradients as for gfront_bwd_persist"""
    T, B, S3 = gates.shape
    S = S3 // 3
    fs = wp.size(0)
    ld = _check_table(((gates, 'gates', (T, B, 3 * S)), (hs, 'hs', (T + 1, B, S)), (gh, 'gh', (T, B, 3 * S)),
                       (whh, 'whh', (3 * S, S)), (wp, 'wp', (fs, S)), (dgi, 'dgi', (T, B, 3 * S)), (dgh, 'dgh', (T, B, 3 * S)),
                       (dxt, 'dxt', (T, B, fs)), (dh_ext, 'dh_ext', (T, B, S)), (x, 'x', (B, T * fs), _PITCHED),
                       (dx_ext, 'dx_ext', (B, T * fs), _PITCHED), (wx, 'wx', (3 * S, fs), _PITCHED)))
    a = _lib.FrontBwdArgs(cell=1, ga=_p(gates), state=_p(hs), gh=_p(gh), x=_p(x), ldx=ld['x'], dh_ext=_p(dh_ext),
                          dx_ext=_p(dx_ext), lddx=ld['dx_ext'], w_hh=_p(whh), w_x=_p(wx), ldwx=ld['wx'], w_p=_p(wp),
                          dgs=_p(dgi), dgh=_p(dgh), dxt=_p(dxt), T=T, B=B, S=S, fs=fs)
    _front_launch('ag_gfront_bwd', a, x.device, _PERSIST_WS_MIN)


def _work_grufront(gates, gh, wx, whh, bhn, wp, *a_, **kw):
    T, B, S3 = gates.shape
    S, fs = S3 // 3, wp.size(0)
    return 'gfront_persist_fwd_kernel<gru>', T * 2.0 * B * (S3 * (S + fs) + fs * S), \
        4.0 * (S3 * (S + fs) + fs * S + T * B * (2 * S3 + 2 * S + fs)), 1


@_timed(_work_grufront)
def grufront_fwd_persist(gates, gh, wx, whh, bhn, wp, bp, hs, x, xt=None):
    """the GRU-front generator's frame loop in ONE persistent launch (ag_gfront_fwd, GRU cell, training); hs: [T,B,S] (h_t);
    x / xt as for gfront_fwd_persist"""
    T, B, S3 = gates.shape
    S = S3 // 3
    fs = wp.size(0)
    ld = _check_table(((gates, 'gates', (T, B, 3 * S)), (gh, 'gh', (T, B, 3 * S)), (whh, 'whh', (3 * S, S)), (bhn, 'bhn', (S,)),
                       (wp, 'wp', (fs, S)), (bp, 'bp', (fs,)), (hs, 'hs', (T, B, S)), (xt, 'xt', (T, B, fs)),
                       (x, 'x', (B, T * fs), _PITCHED), (wx, 'wx', (3 * S, fs), _PITCHED)))
    a = _lib.FrontFwdArgs(cell=1, gen=0, gates=_p(gates), gh=_p(gh), w_x=_p(wx), ldwx=ld['wx'], w_hh=_p(whh), b_hn=_p(bhn),
                          w_p=_p(wp), b_p=_p(bp), hs=_p(hs), x=_p(x), ldx=ld['x'], xt=_p(xt), T=T, B=B, S=S, fs=fs)
    _front_launch('ag_gfront_fwd', a, x.device, int(lib.ag_gfront_persist_ws_bytes(B, S, fs)))


def gfront_gen_persist(pre, wx, whh, wp, bp, ws, bs, u, x, s, first, t_run, bhn=None):
    """the generation mode of the fronts' persistent launch (ag_gfront_fwd, gen = 1): the frame loop of a sample, no history.
    pre [T,B,4S] (LSTM front) or [T,B,3S] (GRU front, then ``bhn`` [S] = b_hh[2S:]) is only read; ws = the stop head's
    weight (S elements), bs [1]; u [T,B] uniforms.  Writes x [B, T*fs] (rows of any pitch: channel 0 of the conv trunk's
    slab), s [B,T] (rows of any pitch >= T), first [B] int32 (frames per clip) and t_run [1] int32 (frames run), all for
    the frames run only (see include/audiogan_hip.h)."""
    T, B, SG = pre.shape
    S = whh.size(1)
    fs = wp.size(0)
    cell = 1 if SG == 3 * S else 0
    assert SG == (3 if cell else 4) * S, (tuple(pre.shape), tuple(whh.shape))
    assert ws.numel() == S, tuple(ws.shape)
    bhn = bhn if cell else None
    ld = _check_table(((pre, 'pre', (T, B, SG)), (whh, 'whh', (SG, S)), (wp, 'wp', (fs, S)), (bp, 'bp', (fs,)),
                       (bs, 'bs', (1,)), (u, 'u', (T, B)), (bhn, 'bhn', (S,)), (ws, 'ws', tuple(ws.shape)),
                       (first, 'first', (B,), torch.int32), (t_run, 't_run', (1,), torch.int32),
                       (x, 'x', (B, T * fs), _PITCHED), (s, 's', (B, T), _PITCHED), (wx, 'wx', (SG, fs), _PITCHED)))
    a = _lib.FrontFwdArgs(cell=cell, gen=1, gates=_p(pre), w_x=_p(wx), ldwx=ld['wx'], w_hh=_p(whh), b_hn=_p(bhn), w_p=_p(wp),
                          b_p=_p(bp), w_s=_p(ws), b_s=_p(bs), u=_p(u), x=_p(x), ldx=ld['x'], s=_p(s), lds=ld['s'],
                          first=_p(first), t_run=_p(t_run), T=T, B=B, S=S, fs=fs)
    _front_launch('ag_gfront_fwd', a, x.device, int(lib.ag_gfront_persist_ws_bytes(B, S, fs)))


# the stacked LSTM front (2 to 8 LSTMCell layers) in one persistent launch; off: one launch per operation and frame
PERSIST_FRONT_STACK = [True]


def gfront_stack_ok(B, S, fs, nl, dev):
    return _persist_ok(lib.ag_gfront_stack_ok, (B, S, fs, nl), dev, PERSIST_FRONT_STACK[0])


def _stack_tables(a, **tables):
    """fills the per-layer pointer tables of a FrontStackArgs (entries past a list's end stay NULL)"""
    for name, lst in tables.items():
        arr = getattr(a, name)
        for i, t in enumerate(lst):
            arr[i] = _p(t)


def _work_gfront_stack(gates, wx, w_in, whh, *a_, **kw):
    """(filed under the name the launch site reported: ag_last_kernel)"""
    nl = len(gates)
    T, B, S4 = gates[0].shape
    S, fs = S4 // 4, wx.size(1)
    return None, T * 2.0 * B * (S4 * (S + fs) + (nl - 1) * S4 * 2 * S + fs * S), \
        4.0 * (S4 * (S + fs) + (nl - 1) * S4 * 2 * S + fs * S + T * B * (nl * (2 * S4 + 2 * S) + fs)), 1


@_timed(_work_gfront_stack)
def gfront_stack_fwd_persist(gates, wx, w_in, whh, bias, wp, bp, hs, cs, x, xt=None):
    """the frame loop of a STACKED LSTM front in ONE persistent launch (ag_gfront_stack_fwd, training).  Lists over the nl
    layers: gates [T,B,4S] (gates[0] holds the z / c pre-activations incl. both biases and, like the others, receives the
    activated gates), whh [4S,S], hs [T,B,S], cs [T+1,B,S]; for the layers from 1 on: w_in (W_ih_l [4S,S]) and bias
    (b_ih_l + b_hh_l [4S]), nl - 1 entries each.  wx = W_ih_0[:, :fs] (any row pitch); x / xt as for gfront_fwd_persist"""
    nl = len(gates)
    T, B, S4 = gates[0].shape
    S = S4 // 4
    fs = wp.size(0)
    assert len(whh) == len(hs) == len(cs) == nl and len(w_in) == len(bias) == nl - 1
    rows = [(wp, 'wp', (fs, S)), (bp, 'bp', (fs,)), (xt, 'xt', (T, B, fs)), (x, 'x', (B, T * fs), _PITCHED),
            (wx, 'wx', (4 * S, fs), _PITCHED)]
    for l in range(nl):
        rows += [(gates[l], 'gates[%d]' % l, (T, B, 4 * S)), (whh[l], 'whh[%d]' % l, (4 * S, S)),
                 (hs[l], 'hs[%d]' % l, (T, B, S)), (cs[l], 'cs[%d]' % l, (T + 1, B, S))]
    for l in range(nl - 1):
        rows += [(w_in[l], 'w_in[%d]' % (l + 1), (4 * S, S)), (bias[l], 'bias[%d]' % (l + 1), (4 * S,))]
    ld = _check_table(rows)
    a = _lib.FrontStackArgs(gen=0, nl=nl, ldwx=ld['wx'], w_p=_p(wp), b_p=_p(bp), x=_p(x), ldx=ld['x'], xt=_p(xt),
                            T=T, B=B, S=S, fs=fs)
    _stack_tables(a, gates=gates, hs=hs, cs=cs, w_hh=whh, w_in=[wx] + list(w_in), bias=[None] + list(bias))
    _front_launch('ag_gfront_stack_fwd', a, x.device, int(lib.ag_gfront_stack_ws_bytes(B, S, fs, nl)))


def gfront_stack_gen_persist(pre, wx, w_in, whh, bias, wp, bp, ws, bs, u, x, s, first, t_run):
    """the generation mode of the stacked front's launch (ag_gfront_stack_fwd, gen = 1): no history.  pre [T,B,4S] (layer 0's
    z / c pre-activations) is only read; whh: nl tensors, w_in / bias: nl - 1 (layers 1 ..); the stop head (ws, bs), the
    uniforms u and the outputs x, s, first, t_run as for gfront_gen_persist"""
    nl = len(whh)
    T, B, S4 = pre.shape
    S = S4 // 4
    fs = wp.size(0)
    assert len(w_in) == len(bias) == nl - 1 and ws.numel() == S, (nl, len(w_in), len(bias), tuple(ws.shape))
    rows = [(pre, 'pre', (T, B, 4 * S)), (wp, 'wp', (fs, S)), (bp, 'bp', (fs,)), (bs, 'bs', (1,)), (u, 'u', (T, B)),
            (ws, 'ws', tuple(ws.shape)), (first, 'first', (B,), torch.int32), (t_run, 't_run', (1,), torch.int32),
            (x, 'x', (B, T * fs), _PITCHED), (s, 's', (B, T), _PITCHED), (wx, 'wx', (4 * S, fs), _PITCHED)]
    for l in range(nl):
        rows.append((whh[l], 'whh[%d]' % l, (4 * S, S)))
    for l in range(nl - 1):
        rows += [(w_in[l], 'w_in[%d]' % (l + 1), (4 * S, S)), (bias[l], 'bias[%d]' % (l + 1), (4 * S,))]
    ld = _check_table(rows)
    a = _lib.FrontStackArgs(gen=1, nl=nl, ldwx=ld['wx'], w_p=_p(wp), b_p=_p(bp), w_s=_p(ws), b_s=_p(bs), u=_p(u), x=_p(x),
                            ldx=ld['x'], s=_p(s), lds=ld['s'], first=_p(first), t_run=_p(t_run), T=T, B=B, S=S, fs=fs)
    _stack_tables(a, gates=[pre], w_hh=whh, w_in=[wx] + list(w_in), bias=[None] + list(bias))
    _front_launch('ag_gfront_stack_fwd', a, x.device, int(lib.ag_gfront_stack_ws_bytes(B, S, fs, nl)))


# the stacked front's backward through time in one persistent launch; off: one launch per operation and frame
PERSIST_FRONT_STACK_BWD = [True]


def gfront_stack_bwd_ok(B, S, fs, nl, dev):
    """(PERSIST_FRONT_BWD: the multi-GPU rule of the one-layer backward holds for this launch too)"""
    return _persist_ok(lib.ag_gfront_stack_bwd_ok, (B, S, fs, nl), dev,
                       PERSIST_FRONT_STACK[0] and PERSIST_FRONT_STACK_BWD[0] and PERSIST_FRONT_BWD[0])


def _work_gfront_stack_bwd(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp, *a_, **kw):
    """(filed under the name the launch site reported: ag_last_kernel)"""
    nl = len(gates)
    T, B, S4 = gates[0].shape
    S, fs = S4 // 4, wp.size(0)
    return None, 2.0 * B * ((T - 1) * S4 * (nl * S + fs) + T * ((nl - 1) * S4 * S + fs * S)), \
        4.0 * (S4 * (nl * S + fs) + (nl - 1) * S4 * S + fs * S + T * B * (nl * (2 * S4 + 2 * S) + S + 3 * fs)), 1


@_timed(_work_gfront_stack_bwd)
def gfront_stack_bwd_persist(gates, cs, x, dh_ext, dx_ext, whh, w_in, wx, wp, dgs, dxt):
    """the backward through time of a STACKED LSTM front in ONE persistent launch (ag_gfront_stack_bwd).  Lists over the nl
    layers: gates [T,B,4S] (activated), cs [T+1,B,S], whh [4S,S], dgs [T,B,4S] (out); w_in: W_ih_l [4S,S] of the layers from
    1 on, nl - 1 entries; wx = W_ih_0[:, :fs] (any row pitch).  dh_ext / dx_ext / x / dxt as for gfront_bwd_persist: the
    external gradients may be None, dh_ext is the TOP layer's"""
    nl = len(gates)
    T, B, S4 = gates[0].shape
    S = S4 // 4
    fs = wp.size(0)
    assert len(cs) == len(whh) == len(dgs) == nl and len(w_in) == nl - 1
    rows = [(wp, 'wp', (fs, S)), (dxt, 'dxt', (T, B, fs)), (dh_ext, 'dh_ext', (T, B, S)), (x, 'x', (B, T * fs), _PITCHED),
            (dx_ext, 'dx_ext', (B, T * fs), _PITCHED), (wx, 'wx', (4 * S, fs), _PITCHED)]
    for l in range(nl):
        rows += [(gates[l], 'gates[%d]' % l, (T, B, 4 * S)), (cs[l], 'cs[%d]' % l, (T + 1, B, S)),
                 (whh[l], 'whh[%d]' % l, (4 * S, S)), (dgs[l], 'dgs[%d]' % l, (T, B, 4 * S))]
    for l in range(nl - 1):
        rows.append((w_in[l], 'w_in[%d]' % (l + 1), (4 * S, S)))
    ld = _check_table(rows)
    a = _lib.FrontStackBwdArgs(nl=nl, w_p=_p(wp), x=_p(x), ldx=ld['x'], dh_ext=_p(dh_ext), dx_ext=_p(dx_ext),
                               lddx=ld['dx_ext'], ldwx=ld['wx'], dxt=_p(dxt), T=T, B=B, S=S, fs=fs)
    _stack_tables(a, ga=gates, cs=cs, w_hh=whh, w_in=[wx] + list(w_in), dgs=dgs)
    _front_launch('ag_gfront_stack_bwd', a, x.device, int(lib.ag_gfront_stack_bwd_ws_bytes(B, S, fs, nl)))


def lstm_persist_bwd_ok(B, H, ndir, dev):
    return _persist_ok(lib.ag_lstm_persist_bwd_ok, (B, H, ndir), dev)


def _work_seq_bwd_persist(gates, whh, c_all, dy, dgates, valid, dgsum=None, dg16=None):
    T, B, H4 = gates[0].shape
    nd = len(gates)
    return 'lstm_persist_bwd_kernel' + _bf16_tag(), T * 2.0 * nd * B * H4 * (H4 // 4), \
        4.0 * nd * (H4 * (H4 // 4) + T * 5.5 * B * H4), 1


@_timed(_work_seq_bwd_persist)
def _lstm_seq_bwd_persist_call(gates, whh, c_all, dy, dgates, valid, dgsum=None, dg16=None):
    """ONE persistent launch for the whole backward through time (ag_lstm_seq_bwd_persist); dgsum: optional list of
    [B,4H] outputs (one per direction) = the sum over time of dgates; dy: fp32 or bf16; dg16: optional list of [T,B,4H]
    bfloat16 outputs = dgates rounded (the operand of the gradient products on bf16 storage)"""
    ndir = len(gates)
    T, B, H4 = gates[0].shape
    H = H4 // 4
    _check_table(_per_dir(ndir, (gates, 'gates', (T, B, 4 * H)), (whh, 'whh', (4 * H, H)), (c_all, 'c_all', (T + 1, B, H)),
                          (dgates, 'dgates', (T, B, 4 * H)), (dgsum, 'dgsum', (B, 4 * H)))
                 + [(dy, 'dy', (T, B, ndir * H), _F32_OR_BF16)])
    _chk(valid, 'valid', torch.int64)
    ld16 = 0
    if dg16 is not None:
        assert len(dg16) == ndir
        for t_ in dg16:      # views [T,B,4H] of one [T,B,ndir*4H] tensor (or separate contiguous tensors): a common row pitch
            _chk(t_, 'dg16', torch.bfloat16)
            assert tuple(t_.shape) == (T, B, 4 * H) and t_.stride(2) == 1 and t_.stride(0) == B * t_.stride(1)
        ld16 = dg16[0].stride(1)
        assert all(t_.stride(1) == ld16 for t_ in dg16)
    ws = _persist_workspace(dy.device, 8192 + 256)
    check(lib.ag_lstm_seq_bwd_persist(_ptr_table(gates), _ptr_table(whh), _ptr_table(c_all), _p(dy), int(_is16(dy)),
                                      _ptr_table(dgates), _ptr_table(dgsum) if dgsum is not None else None,
                                      _ptr_table(dg16) if dg16 is not None else None, ld16, _p(valid),
                                      _p(ws), ws.numel(), T, B, H, ndir, _n_cu(dy.device), _stream()),
          'ag_lstm_seq_bwd_persist')


def _lstm_seq_bwd_range(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, k0, k1, phases=3):
    """steps k1 - 1 .. k0 of the per-step backward, one launch per step and phase (ag_lstm_seq_bwd; phases: 1 = the cell
    backward, 2 = the recurrent product, 3 = both)"""
    ndir = len(gates)
    T, B, H4 = gates[0].shape
    H = H4 // 4
    _check_table(_per_dir(ndir, (gates, 'gates', (T, B, 4 * H)), (whh, 'whh', (4 * H, H)), (c_all, 'c_all', (T + 1, B, H)),
                          (dgates, 'dgates', (T, B, 4 * H)), (dhbuf, 'dhbuf', (2, B, H)), (dcbuf, 'dcbuf', (2, B, H)))
                 + [(dy, 'dy', (T, B, ndir * H))])
    _chk(valid, 'valid', torch.int64)
    _ws = _bind_ws(ndir * lib.ag_skinny_ws_numel(B, H, 4 * H), dy.device) if H % 16 else None  # noqa: F841
    check(lib.ag_lstm_seq_bwd(_ptr_table(gates), _ptr_table(whh), _ptr_table(c_all), _p(dy),
                              _ptr_table(dgates), _ptr_table(dhbuf), _ptr_table(dcbuf), _p(valid), T, B, H,
                              ndir, k0, k1, phases, _stream()), 'ag_lstm_seq_bwd')


# the same call under three names: what lstm_seq_bwd files its launches under when the Profiler is on
def _work_seq_bwd_cell(gates, whh, *a_, **kw):
    T, B, H4 = gates[0].shape
    return 'lstm_cell_bwd2_kernel', 0.0, 4.0 * len(gates) * B * H4 * 3.5


def _work_seq_bwd_prod(gates, whh, *a_, **kw):
    T, B, H4 = gates[0].shape
    nd = len(gates)
    return 'skinny_gemm_kernel', 2.0 * nd * B * H4 * (H4 // 4), 4.0 * nd * (H4 * (H4 // 4) + 2 * B * H4)


def _work_seq_bwd_step(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, k0, k1, *a_, **kw):
    T, B, H4 = gates[0].shape
    nd, n = len(gates), k1 - k0
    return 'lstm_step_bwd_kernel', n * 2.0 * nd * B * H4 * (H4 // 4), n * 4.0 * nd * (H4 * (H4 // 4) + 5.5 * B * H4), n


_lstm_seq_bwd_cell = _timed(_work_seq_bwd_cell, name='_lstm_seq_bwd_cell')(_lstm_seq_bwd_range)
_lstm_seq_bwd_prod = _timed(_work_seq_bwd_prod, name='_lstm_seq_bwd_prod')(_lstm_seq_bwd_range)
_lstm_seq_bwd_step = _timed(_work_seq_bwd_step, name='_lstm_seq_bwd_step')(_lstm_seq_bwd_range)


def lstm_seq_bwd(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, dgsum=None, dg16=None):
    """``dgsum``: optional list of [B,4H] tensors (one per direction) that receive the sum over time of dgates.  Returns True
    when they were filled (the persistent launch sums them in registers); False: the caller sums dgates itself.
    ``dg16`` / a bf16 ``dy``: the persistent launch only (callers check lstm_persist_bwd_ok first)."""
    T = gates[0].size(0)
    if lstm_persist_bwd_ok(gates[0].size(1), gates[0].size(2) // 4, len(gates), dy.device):
        _lstm_seq_bwd_persist_call(gates, whh, c_all, dy, dgates, valid, dgsum, dg16)
        return dgsum is not None
    assert dg16 is None and not _is16(dy), 'bf16 storage needs the persistent launch'

    if Profiler.enabled:
        H = gates[0].size(2) // 4
        if H % 16 == 0:         # the fused step kernel: the whole chain between one pair of events
            _lstm_seq_bwd_step(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, 0, T, 3)
            return
        for k_ in reversed(range(T)):
            _lstm_seq_bwd_cell(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, k_, k_ + 1, 1)
            if k_ > 0:
                _lstm_seq_bwd_prod(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, k_, k_ + 1, 2)
    else:
        _lstm_seq_bwd_range(gates, whh, c_all, dy, dgates, dhbuf, dcbuf, valid, 0, T)
    return False


# ------------------------------------------------------------------------------------
# GRU cell pointwise (config C4)
# ------------------------------------------------------------------------------------
@_timed()
def gru_cell_fwd(gi, gh, h_prev, h_out):
    """gi, gh: [B,3H] contiguous (complete products incl. biases); gi <- (r,z,n); h_out <- h'"""
    for t_, n in ((gi, 'gi'), (gh, 'gh')):
        _chk(t_, n)
        assert t_.is_contiguous()
    B, H3 = gi.shape
    H = H3 // 3
    assert tuple(gh.shape) == (B, H3) and tuple(h_prev.shape) == (B, H) and tuple(h_out.shape) == (B, H)
    check(lib.ag_gru_cell_fwd(_p(gi), _p(gh), _p(h_prev), _mat(h_prev, 'h_prev'), _p(h_out), _mat(h_out, 'h_out'),
                              B, H, _stream()), 'ag_gru_cell_fwd')


@_timed()
def gru_cell_bwd(gates_act, gh, h_prev, dh, dgi, dgh, dh_prev):
    for t_, n in ((gates_act, 'gates_act'), (gh, 'gh'), (dgi, 'dgi'), (dgh, 'dgh')):
        _chk(t_, n)
        assert t_.is_contiguous()
    B, H3 = gates_act.shape
    H = H3 // 3
    check(lib.ag_gru_cell_bwd(_p(gates_act), _p(gh), _p(h_prev), _mat(h_prev, 'h_prev'), _p(dh), _mat(dh, 'dh'),
                              _p(dgi), _p(dgh), _p(dh_prev), _mat(dh_prev, 'dh_prev'), B, H, _stream()),
          'ag_gru_cell_bwd')


@_timed()
def act_bwd2d(dy, y, dx, act, slope=LEAKY_SLOPE):
    """dx = dy * act'(.) on 2-D row-strided views (unit stride along dim 1)"""
    a, b, c = _mat(dy, 'dy'), _mat(y, 'y'), _mat(dx, 'dx')
    assert tuple(dy.shape) == tuple(y.shape) == tuple(dx.shape)
    check(lib.ag_act_bwd2d(_p(dy), a, _p(y), b, _p(dx), c, dy.size(0), dy.size(1), act, slope, _stream()),
          'ag_act_bwd2d')


# ------------------------------------------------------------------------------------
# single-output-channel stride-1 conv (Generator's final conv)
# ------------------------------------------------------------------------------------
def conv_o1_ok(spec_kind, cout, K_, stride, pad):
    return spec_kind == 'conv' and cout == 1 and stride == 1 and K_ <= 9 and 2 * pad == K_ - 1


@_timed()
def conv_o1_fwd(x, w, bias, y, K_, pad, act=ACT_NONE, slope=LEAKY_SLOPE):
    """x [B,C,L] view, w [1,C,K] contiguous, y [B,1,L] view"""
    x_bs, x_cs = _bcl(x, 'x')
    y_bs, _ = _bcl(y, 'y')
    _chk(w, 'w'); _chk(bias, 'bias')
    B, Cc, L = x.shape
    assert w.is_contiguous() and w.numel() == Cc * K_ and tuple(y.shape) == (B, 1, L)
    check(lib.ag_conv1d_o1_fwd(_p(x), x_bs, x_cs, _p(w), _p(bias), _p(y), y_bs, B, Cc, L, K_, pad, act, slope,
                               _stream()), 'ag_conv1d_o1_fwd')


@_timed()
def conv_o1_bwd_data(dy, w, dx, K_, pad, accumulate=False):
    dy_bs, _ = _bcl(dy, 'dy')
    dx_bs, dx_cs = _bcl(dx, 'dx')
    B, Cc, L = dx.shape
    assert w.is_contiguous() and w.numel() == Cc * K_ and tuple(dy.shape) == (B, 1, L)
    check(lib.ag_conv1d_o1_bwd_data(_p(dy), dy_bs, _p(w), _p(dx), dx_bs, dx_cs, B, Cc, L, K_, pad,
                                    int(accumulate), _stream()), 'ag_conv1d_o1_bwd_data')


@_timed()
def conv_o1_wgrad(dy, x, dw, K_, pad):
    dy_bs, _ = _bcl(dy, 'dy')
    x_bs, x_cs = _bcl(x, 'x')
    B, Cc, L = x.shape
    assert dw.is_contiguous() and dw.numel() == Cc * K_ and tuple(dy.shape) == (B, 1, L)
    _ws = _bind_ws(_SMALL_WS, dw.device)  # noqa: F841
    check(lib.ag_conv1d_o1_wgrad(_p(dy), dy_bs, _p(x), x_bs, x_cs, _p(dw), B, Cc, L, K_, pad, _stream()),
          'ag_conv1d_o1_wgrad')


# ------------------------------------------------------------------------------------
# feature-matching statistics over time (calc_dists)
# ------------------------------------------------------------------------------------
def time_moments_fwd(h, lens, m, s, f):
    """h [B,C,L] view (unit stride along L), lens int64 [B]; m, s, f [B,C] contiguous (written)"""
    a = _bcl(h, 'h')
    _chk(lens, 'lens', torch.int64)
    B, Cc, L = h.shape
    for t_, n in ((m, 'm'), (s, 's'), (f, 'f')):
        _chk(t_, n)
        assert t_.is_contiguous() and tuple(t_.shape) == (B, Cc)
    check(lib.ag_time_moments_fwd(_p(h), a[0], a[1], _p(lens), _p(m), _p(s), _p(f), B, Cc, L, _stream()),
          'ag_time_moments_fwd')


def time_moments_bwd(h, lens, gm, gs, gf, dh):
    a, d = _bcl(h, 'h'), _bcl(dh, 'dh')
    _chk(lens, 'lens', torch.int64)
    B, Cc, L = h.shape
    assert tuple(dh.shape) == (B, Cc, L)
    for t_, n in ((gm, 'gm'), (gs, 'gs'), (gf, 'gf')):
        _chk(t_, n)
        assert t_ is None or (t_.is_contiguous() and tuple(t_.shape) == (B, Cc))
    check(lib.ag_time_moments_bwd(_p(h), a[0], a[1], _p(lens), _p(gm), _p(gs), _p(gf), _p(dh), d[0], d[1], B, Cc, L,
                                  _stream()), 'ag_time_moments_bwd')


# ------------------------------------------------------------------------------------
# Conv2DLSTMCell pieces (csrc/convlstm.hip); every map [H, B, C, W] contiguous, peephole weights [H, F, W]
# ------------------------------------------------------------------------------------
def _hbcw(t, name, shape=None):
    _chk(t, name)
    assert t.is_contiguous() and t.dim() == 4, name + ' must be a contiguous [H,B,C,W] map'
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), tuple(shape))
    return t


def _peep(t, name, H, F, W):
    if t is None:
        return None
    _chk(t, name)
    assert t.is_contiguous() and tuple(t.shape) == (H, F, W), (name, tuple(t.shape))
    return t


@_timed()
def convlstm_peephole_fwd(y, c, wci, wcf, j, ip, fp, o):
    H, B, F, W = c.shape
    _hbcw(y, 'y', (H, B, 4 * F, W))
    for t_, n in ((c, 'c'), (j, 'j'), (ip, 'i_pre'), (fp, 'f_pre'), (o, 'o_raw')):
        _hbcw(t_, n, (H, B, F, W))
    check(lib.ag_convlstm_peephole_fwd(_p(y), _p(c), _p(_peep(wci, 'w_ci', H, F, W)), _p(_peep(wcf, 'w_cf', H, F, W)), _p(j),
                                       _p(ip), _p(fp), _p(o), H, B, F, W, _stream()), 'ag_convlstm_peephole_fwd')


@_timed()
def convlstm_peephole_bwd(dj, di, df, do, c, wci, wcf, dy, dc, dwci, dwcf):
    """dy [H,B,4F,W] written; dc accumulated into; dwci / dwcf written when given"""
    H, B, F, W = c.shape
    _hbcw(dy, 'dy', (H, B, 4 * F, W))
    for t_, n in ((dj, 'dj'), (di, 'di'), (df, 'df'), (do, 'do'), (c, 'c'), (dc, 'dc')):
        _hbcw(t_, n, (H, B, F, W))
    check(lib.ag_convlstm_peephole_bwd(_p(dj), _p(di), _p(df), _p(do), _p(c), _p(_peep(wci, 'w_ci', H, F, W)),
                                       _p(_peep(wcf, 'w_cf', H, F, W)), _p(dy), _p(dc), _p(_peep(dwci, 'dw_ci', H, F, W)),
                                       _p(_peep(dwcf, 'dw_cf', H, F, W)), H, B, F, W, _stream()), 'ag_convlstm_peephole_bwd')


@_timed()
def convlstm_cell_fwd(j, i_, f_, c, o_raw, wco, forget_bias, c_new, o_pre):
    H, B, F, W = c.shape
    for t_, n in ((j, 'j'), (i_, 'i'), (f_, 'f'), (c, 'c'), (o_raw, 'o_raw'), (c_new, 'c_new'), (o_pre, 'o_pre')):
        _hbcw(t_, n, (H, B, F, W))
    check(lib.ag_convlstm_cell_fwd(_p(j), _p(i_), _p(f_), _p(c), _p(o_raw), _p(_peep(wco, 'w_co', H, F, W)), float(forget_bias),
                                   _p(c_new), _p(o_pre), H, B, F, W, _stream()), 'ag_convlstm_cell_fwd')


@_timed()
def convlstm_cell_bwd(j, i_, f_, c, c_new, wco, forget_bias, dc_new, do_pre, dj, di, df, dc, dwco):
    """dc_new: in = dL/dc', out = dL/dc' + do_pre * W_co; dj, di, df, dc written; dwco written when given"""
    H, B, F, W = c.shape
    for t_, n in ((j, 'j'), (i_, 'i'), (f_, 'f'), (c, 'c'), (c_new, 'c_new'), (dc_new, 'dc_new'), (do_pre, 'do_pre'),
                  (dj, 'dj'), (di, 'di'), (df, 'df'), (dc, 'dc')):
        _hbcw(t_, n, (H, B, F, W))
    check(lib.ag_convlstm_cell_bwd(_p(j), _p(i_), _p(f_), _p(c), _p(c_new), _p(_peep(wco, 'w_co', H, F, W)), float(forget_bias),
                                   _p(dc_new), _p(do_pre), _p(dj), _p(di), _p(df), _p(dc), _p(_peep(dwco, 'dw_co', H, F, W)),
                                   H, B, F, W, _stream()), 'ag_convlstm_cell_bwd')


@_timed()
def convlstm_out_fwd(o, c, h):
    for t_, n in ((o, 'o'), (c, 'c'), (h, 'h')):
        _chk(t_, n)
        assert t_.is_contiguous() and t_.numel() == o.numel()
    check(lib.ag_convlstm_out_fwd(_p(o), _p(c), _p(h), o.numel(), _stream()), 'ag_convlstm_out_fwd')


@_timed()
def convlstm_out_bwd(o, c, dh, do, dc):
    for t_, n in ((o, 'o'), (c, 'c'), (dh, 'dh'), (do, 'do'), (dc, 'dc')):
        _chk(t_, n)
        assert t_.is_contiguous() and t_.numel() == o.numel()
    check(lib.ag_convlstm_out_bwd(_p(o), _p(c), _p(dh), _p(do), _p(dc), o.numel(), _stream()), 'ag_convlstm_out_bwd')


@_timed()
def layer_norm_hbfw_fwd(x, gamma, beta, eps, y, mean, rstd):
    H, B, F, W = x.shape
    _hbcw(x, 'x'); _hbcw(y, 'y', x.shape)
    for t_, n, k in ((gamma, 'gamma', F), (beta, 'beta', F), (mean, 'mean', B), (rstd, 'rstd', B)):
        _chk(t_, n)
        assert t_.is_contiguous() and t_.numel() == k, n
    check(lib.ag_layer_norm_hbfw_fwd(_p(x), _p(gamma), _p(beta), float(eps), _p(y), _p(mean), _p(rstd), H, B, F, W, _stream()),
          'ag_layer_norm_hbfw_fwd')


@_timed()
def layer_norm_hbfw_bwd(dy, x, gamma, mean, rstd, dx, dgp, dbp):
    H, B, F, W = x.shape
    _hbcw(x, 'x'); _hbcw(dy, 'dy', x.shape); _hbcw(dx, 'dx', x.shape)
    for t_, n, k in ((gamma, 'gamma', F), (mean, 'mean', B), (rstd, 'rstd', B), (dgp, 'dgamma_part', B * F), (dbp, 'dbeta_part', B * F)):
        _chk(t_, n)
        assert t_.is_contiguous() and t_.numel() == k, n
    check(lib.ag_layer_norm_hbfw_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgp), _p(dbp), H, B, F, W, _stream()),
          'ag_layer_norm_hbfw_bwd')


# ------------------------------------------------------------------------------------
# per-iteration summaries (audiogan.py:776-809, :875-884, :911-920) as device scalars + the ring row that gathers them
# ------------------------------------------------------------------------------------
SUMMARY_COLS = _lib.SUMMARY_COLS


def _small_out(out, n, dev, name):
    if out is None:
        return torch.empty(n, dtype=torch.float32, device=dev)
    _chk(out, name)
    assert out.is_contiguous() and out.numel() == n, (name, tuple(out.shape))
    return out


@_timed(_work_named)
def logit_summary(cls, nframes, positive, out=None):
    """one critic output cls [B,T'] (fp32, any strides: ``Discriminator.classify`` returns a transposed view) ->
    out [5] = (mean, std, hits, mask sum, hits / mask sum): mean / std over all B*T' entries, population (numpy's
    ``.mean()`` / ``.std()``, audiogan.py:799-802); hits = entries inside ``nframes`` with cls > 0 (``positive``) or < 0
    (ag_logit_summary: one launch, two-pass variance, fixed-order sums)"""
    _chk(cls, 'cls'); _chk(nframes, 'nframes', torch.int64)
    assert cls.dim() == 2, tuple(cls.shape)
    B, T = cls.shape
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    out = _small_out(out, 5, cls.device, 'out')
    check(lib.ag_logit_summary(_p(cls), cls.stride(0), cls.stride(1), _p(nframes), int(bool(positive)), _p(out), B, T,
                               _stream()), 'ag_logit_summary')
    return out


@_timed(_work_named)
def sqnorm_rows(gx, nframes, scale, part=None, out=None, finish=True):
    """gx [B,L] (unit stride along L, any row pitch; 16-byte aligned rows are read four at a time) ->
    part[b] = scale * sum_l gx[b,l]^2 / nframes[b].  ``finish``: a second launch writes out[0] = mean_b part[b] (b ascending);
    False: the caller hands ``part`` to ``summary_commit``, which takes the same mean.  Returns (part, out or None)."""
    B, L = gx.shape
    ld = _rows(gx, 'gx', B, L)
    _chk(nframes, 'nframes', torch.int64)
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    part = _small_out(part, B, gx.device, 'part')
    if finish:
        out = _small_out(out, 1, gx.device, 'out')
    else:
        assert out is None
    check(lib.ag_sqnorm_rows(_p(gx), ld, _p(nframes), float(scale), _p(part), _p(out), B, L, _stream()), 'ag_sqnorm_rows')
    return part, out


@_timed(_work_named)
def vec_stats(v, sign=1.0, out=None):
    """v [n] contiguous -> out [2] = (sign * mean(v), population std(v)) (ag_vec_stats; reward/mean, reward/std of :879-880)"""
    _chk(v, 'v')
    assert v.dim() == 1 and v.is_contiguous() and v.numel() > 0, tuple(v.shape)
    out = _small_out(out, 2, v.device, 'out')
    check(lib.ag_vec_stats(_p(v), float(sign), _p(out), v.numel(), _stream()), 'ag_vec_stats')
    return out


def persist_status_word(dev):
    """the sticky status word of the CURRENT persistent workspace on ``dev`` as an int32 [1] view (None: no persistent
    launch has run there yet)"""
    dev = torch.device(dev)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    lst = _persist_ws.get(dev, [])
    return lst[0][:4].view(torch.int32) if lst else None


@_timed(_work_named)
def summary_commit(ring, cursor, cols, part=None, part_col=-1):
    """one row of the summary ring in one launch (ag_summary_commit).  ring: int32 [capacity, 16] contiguous; cursor: int32
    [2] (next row, next sequence number; both advanced by the launch); cols: 16 entries, each a one-element float32 / int32
    device tensor (its 32-bit word is copied as it is), a Python int (int32 bits), a float (fp32 bits) or None (0) - column
    1 is overwritten by the sequence number; part / part_col: column ``part_col`` = mean of the fp32 vector ``part`` (b
    ascending, what ``sqnorm_rows(finish=True)`` computes).  The descriptor goes through the table arena: a captured launch
    keeps reading its device copy on every replay."""
    import struct
    _chk(ring, 'ring', torch.int32); _chk(cursor, 'cursor', torch.int32); _chk(part, 'part')
    assert ring.dim() == 2 and ring.size(1) == SUMMARY_COLS and ring.is_contiguous() and ring.size(0) >= 1
    assert cursor.is_contiguous() and cursor.numel() == 2 and len(cols) == SUMMARY_COLS
    d = _lib.SummaryDesc()
    for i, c in enumerate(cols):
        if torch.is_tensor(c):
            if not c.is_cuda:
                raise RuntimeError('audiogan_amd: summary column %d must be a CUDA (HIP) tensor; there is no CPU path' % i)
            if c.dtype not in (torch.float32, torch.int32) or c.numel() != 1:
                raise TypeError('audiogan_amd: summary column %d must be one float32 / int32 element, got %s %r'
                                % (i, c.dtype, tuple(c.shape)))
            d.src[i] = c.data_ptr()
        elif isinstance(c, float):
            d.imm[i] = struct.unpack('<I', struct.pack('<f', c))[0]
        elif c is not None:
            d.imm[i] = int(c) & 0xFFFFFFFF
    if part is not None:
        assert part.is_contiguous() and part.dim() == 1 and 0 <= part_col < SUMMARY_COLS
        d.part, d.npart, d.part_col = part.data_ptr(), part.numel(), int(part_col)
    else:
        d.part_col = -1
    d.ring, d.cursor, d.capacity = ring.data_ptr(), cursor.data_ptr(), ring.size(0)
    tab = _table('summary', [d], ring.device)
    check(lib.ag_summary_commit(_p(tab), _stream()), 'ag_summary_commit')


# ------------------------------------------------------------------------------------
# held-out evaluation (evaluate.Evaluator): long-term average spectrum of ragged clips, running critic statistics
# ------------------------------------------------------------------------------------
LTAS_BINS = 129          # bins 0..128 of the 256-point DFT
SCORE_WORDS = 6


@_timed(_work_named)
def ltas_power(x, lens, out=None, nframes=None):
    """x [B, L] (unit stride along L, any row pitch), lens int64 [B] or None -> out [B, 129] fp32: per clip the mean over its
    frames (256 samples, hop 128, periodic Hann; a clip shorter than one frame is ONE zero-padded frame) of the power
    |X[k]|^2 of the 256-point DFT, k = 0..128.  ``nframes``: an int32 [B] tensor that receives the frame counts.  Samples at
    or past ``lens`` are never read.  Returns ``out``; the logarithm is the caller's (ag_ltas_power)."""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64); _chk(nframes, 'nframes', torch.int32)
    assert x.dim() == 2, tuple(x.shape)
    B, L = x.shape
    ld = _rows(x, 'x', B, L)
    assert lens is None or (lens.is_contiguous() and lens.numel() == B)
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    if out is None:
        out = torch.empty(B, LTAS_BINS, dtype=torch.float32, device=x.device)
    _chk(out, 'out')
    assert out.is_contiguous() and tuple(out.shape) == (B, LTAS_BINS), tuple(out.shape)
    _bind_ws(int(lib.ag_ltas_ws_numel(B, L)), x.device)         # (both launches are enqueued before the call returns)
    check(lib.ag_ltas_power(_p(x), ld, _p(lens), _p(out), _p(nframes), B, L, _stream()), 'ag_ltas_power')
    return out


@_timed(_work_named)
def score_accum(cls, nframes, target, positive, acc):
    """one critic output cls [B, T'] (fp32, any strides) ADDED to ``acc``, six float64 device words the caller zeroes once per
    evaluation: clips with a valid frame, sum_b of the per-clip mean BCE towards ``target``, valid frames, hits among them
    (cls > 0 if ``positive`` else cls < 0), sum cls, sum cls^2 over the valid frames (ag_score_accum: one launch, sums in
    double, masked entries never read)."""
    _chk(cls, 'cls'); _chk(nframes, 'nframes', torch.int64); _chk(acc, 'acc', torch.float64)
    assert cls.dim() == 2, tuple(cls.shape)
    B, T = cls.shape
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    assert acc.is_contiguous() and acc.numel() == SCORE_WORDS, tuple(acc.shape)
    check(lib.ag_score_accum(_p(cls), cls.stride(0), cls.stride(1), _p(nframes), float(target), int(bool(positive)), _p(acc),
                             B, T, _stream()), 'ag_score_accum')
    return acc


# ------------------------------------------------------------------------------------
# aligned distance (evaluate.Evaluator(aligned=True), evaluate.aligned_distance): per-frame mel cepstra, DTW totals
# ------------------------------------------------------------------------------------
MEL_BANDS, MEL_NCEP, CEP_WIDTH = 24, 13, 16          # columns 0..12 of a 16-float row hold the cepstra, 13..15 are zero
DTW_MAX_FRAMES = 1024
_ALIGN_TABLES = {}


def lt_frames(L):
    """frames of a clip of L samples (256 samples, hop 128; a clip shorter than one frame is one zero-padded frame)"""
    return (int(L) - 256) // 128 + 1 if L >= 256 else 1


def _mel64(sr, bands):
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)          # noqa: E731
    edges = 700.0 * (10.0 ** (np.linspace(0.0, mel(sr / 2.0), bands + 2) / 2595.0) - 1.0)
    f = np.arange(LTAS_BINS, dtype=np.float64) * sr / 256.0
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    return np.maximum(0.0, np.minimum((f[None, :] - lo) / (mid - lo), (hi - f[None, :]) / (hi - mid)))


def _dct64(bands, ncep):
    q, m = np.arange(ncep, dtype=np.float64)[:, None], np.arange(bands, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / bands) * np.cos(np.pi * q * (m + 0.5) / bands)


def _align_table(key, make, device):
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = key + (str(device),)
    if key not in _ALIGN_TABLES:
        _ALIGN_TABLES[key] = torch.from_numpy(make().astype(np.float32)).to(device)
    return _ALIGN_TABLES[key]


def mel_table(sr=8000, bands=MEL_BANDS, device='cuda'):
    """[bands, 129] fp32: triangles of peak 1 over the bin frequencies k sr / 256, edges equally spaced in
    mel(f) = 2595 log10(1 + f / 700) on [0, mel(sr / 2)]; evaluated in float64, rounded once; cached per device"""
    return _align_table(('mel', int(sr), int(bands)), lambda: _mel64(float(sr), int(bands)), device)


def dct_table(bands=MEL_BANDS, ncep=MEL_NCEP, device='cuda'):
    """[ncep, bands] fp32: sqrt(2 / bands) cos(pi q (m + 0.5) / bands); evaluated in float64, rounded once; cached per device"""
    return _align_table(('dct', int(bands), int(ncep)), lambda: _dct64(int(bands), int(ncep)), device)


@_timed(_work_named)
def melcep_frames(x, lens, mel=None, dct=None, cep=None, nframes=None, power=None):
    """x [B, L] and lens as ``ltas_power`` takes them -> cep [B, F, 16] fp32, F = lt_frames(L): per frame (256 samples, hop 128,
    periodic Hann) the 13 mel cepstra c[q] = sum_m dct[q, m] log(sum_k mel[m, k] |X[k]|^2 + 1e-10) in columns 0..12, zeros
    in 13..15.  ``mel`` [24, 129] / ``dct`` [13, 24]: device tables (default: ``mel_table`` / ``dct_table``); ``nframes``: an
    int32 [B] tensor that receives the frame counts; ``power``: a [B, F, 129] tensor that receives |X[k]|^2 per frame.
    Rows at or past a clip's frame count are not written in either output.  The DFT is an fp32 MFMA product
    (ag_melcep_frames: one launch)."""
    _chk(x, 'x'); _chk(lens, 'lens', torch.int64); _chk(nframes, 'nframes', torch.int32)
    assert x.dim() == 2, tuple(x.shape)
    B, L = x.shape
    ld = _rows(x, 'x', B, L)
    F = lt_frames(L)
    mel = mel_table(device=x.device) if mel is None else mel
    dct = dct_table(device=x.device) if dct is None else dct
    _chk(mel, 'mel'); _chk(dct, 'dct')
    assert mel.is_contiguous() and tuple(mel.shape) == (MEL_BANDS, LTAS_BINS), tuple(mel.shape)
    assert dct.is_contiguous() and tuple(dct.shape) == (MEL_NCEP, MEL_BANDS), tuple(dct.shape)
    assert lens is None or (lens.is_contiguous() and lens.numel() == B)
    assert nframes is None or (nframes.is_contiguous() and nframes.numel() == B)
    if cep is None:
        cep = torch.empty(B, F, CEP_WIDTH, dtype=torch.float32, device=x.device)
    _chk(cep, 'cep'); _chk(power, 'power')
    assert cep.is_contiguous() and tuple(cep.shape) == (B, F, CEP_WIDTH), tuple(cep.shape)
    assert power is None or (power.is_contiguous() and tuple(power.shape) == (B, F, LTAS_BINS)), tuple(power.shape)
    check(lib.ag_melcep_frames(_p(x), ld, _p(lens), _p(mel), _p(dct), _p(cep), _p(nframes), _p(power), B, L, _stream()),
          'ag_melcep_frames')
    return cep


@_timed(_work_named)
def dtw_cost(cep_a, nf_a, cep_b, nf_b, out=None):
    """cep_a [B, Fa, 16], cep_b [B, Fb, 16] (``melcep_frames`` rows), nf_a / nf_b int32 [B] -> out [B] fp32: the total of the
    symmetric dynamic-time-warping recursion D(i, j) = min(D(i-1, j) + d, D(i, j-1) + d, D(i-1, j-1) + 2 d), D(0, 0) = 2 d,
    d the Euclidean distance of columns 1..12, at (n - 1, m - 1).  Every path has weight n + m: divide by it.  Rows at or
    past the counts and columns 0, 13..15 are never read; at most 1024 frames a side (ag_dtw_cost: one launch)."""
    _chk(cep_a, 'cep_a'); _chk(cep_b, 'cep_b'); _chk(nf_a, 'nf_a', torch.int32); _chk(nf_b, 'nf_b', torch.int32)
    assert cep_a.dim() == 3 and cep_b.dim() == 3 and cep_a.size(2) == cep_b.size(2) == CEP_WIDTH, (cep_a.shape, cep_b.shape)
    B, Fa, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(1)
    assert cep_b.size(0) == B and cep_a.is_contiguous() and cep_b.is_contiguous()
    assert nf_a is None or (nf_a.is_contiguous() and nf_a.numel() == B)
    assert nf_b is None or (nf_b.is_contiguous() and nf_b.numel() == B)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=cep_a.device)
    _chk(out, 'out')
    assert out.is_contiguous() and tuple(out.shape) == (B,), tuple(out.shape)
    check(lib.ag_dtw_cost(_p(cep_a), _p(nf_a), _p(cep_b), _p(nf_b), _p(out), B, Fa, Fb, _stream()), 'ag_dtw_cost')
    return out


@_timed(_work_named)
def dtw_pairs(cep_a, nf_a, cep_b, nf_b, ia=None, ib=None, out=None):
    """cep_a [Na, Fa, 16], cep_b [Nb, Fb, 16] (``melcep_frames`` rows), nf_a [Na] / nf_b [Nb] int32: two BANKS of sequences.
    ``ia``, ``ib`` (int32 [P], both or neither) -> out [P] fp32, out[p] = the ``dtw_cost`` total of a[ia[p]] against b[ib[p]]
    (the kernel clamps the indices into the banks); without them -> out [Na, Nb], every a against every b.  The bits are
    those ``dtw_cost`` gives for the same two sequences, and no gathered copy of a bank is made.  Capacities of at most 64
    frames on one side and 256 on the other run one wave per pair; anything else, up to 1024 frames a side, one workgroup
    per pair (ag_dtw_pairs: one launch)."""
    _chk(cep_a, 'cep_a'); _chk(cep_b, 'cep_b'); _chk(nf_a, 'nf_a', torch.int32); _chk(nf_b, 'nf_b', torch.int32)
    _chk(ia, 'ia', torch.int32); _chk(ib, 'ib', torch.int32)
    assert cep_a.dim() == 3 and cep_b.dim() == 3 and cep_a.size(2) == cep_b.size(2) == CEP_WIDTH, (cep_a.shape, cep_b.shape)
    Na, Fa, Nb, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(0), cep_b.size(1)
    assert cep_a.is_contiguous() and cep_b.is_contiguous()
    assert nf_a is None or (nf_a.is_contiguous() and nf_a.numel() == Na)
    assert nf_b is None or (nf_b.is_contiguous() and nf_b.numel() == Nb)
    if (ia is None) != (ib is None):
        raise ValueError('audiogan_amd: dtw_pairs takes ia and ib together or neither')
    if ia is None:
        shape = (Na, Nb)
    else:
        assert ia.dim() == 1 and ia.is_contiguous() and ib.is_contiguous() and ib.shape == ia.shape, (ia.shape, ib.shape)
        shape = (ia.numel(),)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=cep_a.device)
    _chk(out, 'out')
    assert out.is_contiguous() and tuple(out.shape) == shape, (tuple(out.shape), shape)
    check(lib.ag_dtw_pairs(_p(cep_a), _p(nf_a), Na, Fa, _p(cep_b), _p(nf_b), Nb, Fb, _p(ia), _p(ib), _p(out), out.numel(),
                           _stream()), 'ag_dtw_pairs')
    return out


def dtw_align_ws(Fa, Fb):
    """bytes of decision workspace ``dtw_align`` needs PER PAIR at these capacities (two bits per cell; 0: outside 1..1024)"""
    return int(lib.ag_dtw_align_ws(int(Fa), int(Fb)))


# Not under @_timed: tests/test_launch_layer.py pins the timed set, and this launch belongs to data preparation (ingest
# --utterances), which no Profiler run of training or evaluation covers.  tools/prof_dtwalign.py times it with device
# events; the library reports it to ag_last_kernel as "dtw_align_kernel" like every other launch.
def dtw_align(cep_a, nf_a, cep_b, nf_b, total=None, lo=None, hi=None, workspace=None):
    """``dtw_cost`` with its path.  cep_a [B, Fa, 16] (the utterance: rows), cep_b [B, Fb, 16] (the reference: columns), nf_a /
    nf_b int32 [B] or None -> (total [B] fp32, lo [B, Fb] int32, hi [B, Fb] int32): ``total`` has the bits of ``dtw_cost``;
    lo[b, j] / hi[b, j] are the first / last row of a that the optimal path matches to column j, for j < nf_b[b] - columns at
    or past the count are not written.  Ties go to the diagonal, then to (i-1, j), then to (i, j-1).  ``workspace``: a
    device tensor of at least B * dtw_align_ws(Fa, Fb) bytes (default: allocated here) that receives two bits per cell
    (ag_dtw_align: one launch, one workgroup per pair)."""
    assert cep_a.dim() == 3 and cep_b.dim() == 3, (tuple(cep_a.shape), tuple(cep_b.shape))
    B, Fa, Fb = cep_a.size(0), cep_a.size(1), cep_b.size(1)
    dev = cep_a.device
    if total is None:
        total = torch.empty(B, dtype=torch.float32, device=dev)
    if lo is None:
        lo = torch.empty(B, Fb, dtype=torch.int32, device=dev)
    if hi is None:
        hi = torch.empty(B, Fb, dtype=torch.int32, device=dev)
    need = B * dtw_align_ws(Fa, Fb)
    if workspace is None:
        workspace = torch.empty(max(need, 4) // 4, dtype=torch.int32, device=dev)
    _check_table([(cep_a, 'cep_a', (B, Fa, CEP_WIDTH)), (cep_b, 'cep_b', (B, Fb, CEP_WIDTH)),
                  (nf_a, 'nf_a', (B,), torch.int32), (nf_b, 'nf_b', (B,), torch.int32), (total, 'total', (B,)),
                  (lo, 'lo', (B, Fb), torch.int32), (hi, 'hi', (B, Fb), torch.int32)])
    if not workspace.is_cuda:
        raise RuntimeError('audiogan_amd: workspace must be a CUDA (HIP) tensor; there is no CPU path')
    assert workspace.is_contiguous() and workspace.data_ptr() % 4 == 0, 'workspace'
    check(lib.ag_dtw_align(_p(cep_a), _p(nf_a), _p(cep_b), _p(nf_b), _p(total), _p(lo), _p(hi), _p(workspace),
                           workspace.numel() * workspace.element_size(), B, Fa, Fb, _stream()), 'ag_dtw_align')
    return total, lo, hi


# ------------------------------------------------------------------------------------
# pitch measures (evaluate.Evaluator(aligned=True, pitch=True), evaluate.pitch_distance): pitch candidates per frame, the sums
# along the alignment path.  Not under @_timed, as dtw_align is not: tests/test_launch_layer.py pins the timed set;
# tools/prof_pitch.py times them with device events and the library names both launches to ag_last_kernel.
# ------------------------------------------------------------------------------------
PITCH_W, PITCH_TMIN, PITCH_TMAX = int(lib.ag_pitch_window()), int(lib.ag_pitch_tmin()), int(lib.ag_pitch_tmax())
PITCH_LAG0 = PITCH_TMIN - 1                                # the lag of nccf's column 0
PITCH_LAGS = PITCH_TMAX - PITCH_TMIN + 3                   # lags 19..128
PITCH_NCCF = int(lib.ag_pitch_nccf_width())                # floats per nccf row: the lags and two zero columns
PITCH_TILE = int(lib.ag_pitch_tile())                      # frames one workgroup of ag_pitch_frames takes
PITCH_PATH_WORDS = int(lib.ag_pitch_path_words())          # cells, both voiced, voicing differs, gross, sum d^2
PITCH_GROSS = 1200.0 * float(np.log2(1.2))                 # cents: the usual 20 % gross-error threshold
assert (PITCH_W, PITCH_TMIN, PITCH_TMAX, PITCH_LAGS, PITCH_NCCF, PITCH_PATH_WORDS) == (256, 20, 127, 110, 112, 5)


def pitch_frames(x, lens, octf=0.9, center=True, lag=None, peak=None, nccf=None, nframes=None):
    """x [B, L] and lens as ``melcep_frames`` takes them, on ITS framing (frame j starts at sample 128 j; F = lt_frames(L))
    -> (lag [B, F] int32, peak [B, F, 4] fp32).  Per frame the normalised cross-correlation phi(tau) of the 256-sample
    window with its copy tau samples later, tau = 19..128, fp32 fmaf chains in ascending order; ``center``: the mean of the
    segment's valid samples is subtracted first.  lag = the SMALLEST tau in 20..127 that is a local maximum of phi and
    reaches ``octf`` times the largest phi of that range (0: none); peak = phi(lag - 1), phi(lag), phi(lag + 1) and the
    window's mean power e0 / 256.  ``nccf``: a [B, F, 112] tensor that receives phi(19..128) and two zero columns;
    ``nframes``: an int32 [B] tensor that receives the frame counts.  Rows at or past a clip's frame count are not written
    and samples at or past ``lens`` are never read (ag_pitch_frames: one launch; ``evaluate.pitch_cents`` refines)."""
    _chk(x, 'x')
    assert x.dim() == 2, tuple(x.shape)
    B, L = x.shape
    F = lt_frames(L)
    if lag is None:
        lag = torch.empty(B, F, dtype=torch.int32, device=x.device)
    if peak is None:
        peak = torch.empty(B, F, 4, dtype=torch.float32, device=x.device)
    ld = _check_table([(x, 'x', (B, L), _PITCHED), (lens, 'lens', (B,), torch.int64), (lag, 'lag', (B, F), torch.int32),
                       (peak, 'peak', (B, F, 4)), (nccf, 'nccf', (B, F, PITCH_NCCF)),
                       (nframes, 'nframes', (B,), torch.int32)])
    check(lib.ag_pitch_frames(_p(x), ld['x'], _p(lens), float(octf), int(bool(center)), _p(lag), _p(peak), _p(nccf),
                              _p(nframes), B, L, _stream()), 'ag_pitch_frames')
    return lag, peak


def pitch_path_accum(pc_a, pc_b, lo, hi, nf_b=None, gross=None, out=None):
    """pc_a [B, Fa] (the rows of the alignment), pc_b [B, Fb] (its columns): fp32 cents per frame, negative = unvoiced
    (``evaluate.pitch_cents``); lo, hi int32 [B, Fb] and nf_b int32 [B] as ``dtw_align`` leaves and takes them -> out [B, 5]
    fp32: over the path's cells (column j < nf_b[b], rows lo..hi) their number, those with both frames voiced, those whose
    voicing differs, the both-voiced ones further apart than ``gross`` cents (default 1200 log2(1.2)), and the sum of
    (a - b)^2 over the both-voiced ones.  Columns at or past the count are never read; at most 1024 frames a side
    (ag_pitch_path_accum: one launch, one workgroup per pair)."""
    assert pc_a.dim() == 2 and pc_b.dim() == 2, (tuple(pc_a.shape), tuple(pc_b.shape))
    B, Fa, Fb = pc_a.size(0), pc_a.size(1), pc_b.size(1)
    if out is None:
        out = torch.empty(B, PITCH_PATH_WORDS, dtype=torch.float32, device=pc_a.device)
    _check_table([(pc_a, 'pc_a', (B, Fa)), (pc_b, 'pc_b', (B, Fb)), (lo, 'lo', (B, Fb), torch.int32),
                  (hi, 'hi', (B, Fb), torch.int32), (nf_b, 'nf_b', (B,), torch.int32), (out, 'out', (B, PITCH_PATH_WORDS))])
    check(lib.ag_pitch_path_accum(_p(pc_a), _p(pc_b), _p(lo), _p(hi), _p(nf_b), float(PITCH_GROSS if gross is None else gross),
                                  _p(out), B, Fa, Fb, _stream()), 'ag_pitch_path_accum')
    return out


# ------------------------------------------------------------------------------------
# ingestion (audio.resample, ingest.build_store): polyphase resampling of ragged rows of PCM frames
# ------------------------------------------------------------------------------------
def resample_ok(L, M, taps, channels, kind):
    """the library's rule for ag_resample_poly: L taps 4 <= 64 KB, taps odd and >= 3, 1..8 channels, kind 0 (fp32) / 1 (int16)"""
    return bool(lib.ag_resample_ok(int(L), int(M), int(taps), int(channels), int(kind)))


@_timed(_work_named)
def resample_poly(src, src_len, bank, L, M, dst=None, n_out=None, in_start=0, out_start=0):
    """src [B, n_in] or [B, n_in, C] (fp32 or int16; unit stride along the channels, C along the frames, any row pitch):
    frames in_start .. in_start + len_b - 1 of B signals, len_b = clamp(src_len[b], 0, n_in) (int64 [B] or None: n_in);
    ``bank`` [L, taps] fp32 (``audio.resample_bank``).  -> (dst [B, n_out] fp32, counts int64 [B] = ceil(len_b L / M)):
    dst[b, n] = y[out_start + n], y[N] = sum_t bank[p, t] x[base - half + t], base = (N M) div L, p = (N M) mod L, x the mono
    signal (channels averaged in fp32, int16 times 2^-15), zero outside the row's frames.  ``n_out`` defaults to
    ceil(n_in L / M); ALL n_out entries of every row are written - slice at the counts.  A chunk of a signal (its two
    starts set) has the bits of the whole (ag_resample_poly: one launch)."""
    kind = 1 if src.dtype == torch.int16 else 0
    _chk(src, 'src', torch.int16 if kind else torch.float32); _chk(src_len, 'src_len', torch.int64); _chk(bank, 'bank')
    assert src.dim() in (2, 3), tuple(src.shape)
    B, n_in = src.size(0), src.size(1)
    C = src.size(2) if src.dim() == 3 else 1
    if src.dim() == 3:
        assert (C == 1 or src.stride(2) == 1) and (n_in <= 1 or src.stride(1) == C), (tuple(src.shape), src.stride())
    else:
        assert n_in <= 1 or src.stride(1) == 1, (tuple(src.shape), src.stride())
    pitch = src.stride(0) if B > 1 else max(src.stride(0), n_in * C)
    assert bank.dim() == 2 and bank.is_contiguous() and tuple(bank.shape)[0] == L, (tuple(bank.shape), L)
    assert src_len is None or (src_len.is_contiguous() and src_len.numel() == B)
    if n_out is None:
        n_out = dst.size(1) if dst is not None else (n_in * L + M - 1) // M
    if dst is None:
        dst = torch.empty(B, n_out, dtype=torch.float32, device=src.device)
    ldd = _rows(dst, 'dst', B, n_out)
    check(lib.ag_resample_poly(_p(src), kind, C, pitch, _p(src_len), n_in, int(in_start), _p(bank), int(L), int(M),
                               bank.size(1), _p(dst), ldd, n_out, int(out_start), B, _stream()), 'ag_resample_poly')
    if src_len is None:
        counts = torch.full((B,), (n_in * L + M - 1) // M, dtype=torch.int64, device=src.device)
    else:
        counts = (src_len.clamp(0, n_in) * L + (M - 1)) // M
    return dst, counts


# ------------------------------------------------------------------------------------
# the device-resident word store (dataset.DeviceWordStore, dataset.ClipBatch): clip facts once, one gather per minibatch
# ------------------------------------------------------------------------------------
def _clip_store(bank, start, cap_or_n, second):
    """the checks both launches share: a 16-byte aligned fp32 bank of a multiple of 4 floats, int64 starts, one int32 per clip"""
    _chk(bank, 'bank'); _chk(start, 'start', torch.int64); _chk(cap_or_n, second, torch.int32)
    if bank.dim() != 1 or not bank.is_contiguous() or bank.numel() % 4 or bank.data_ptr() % 16:
        raise ValueError('audiogan_amd: the clip bank must be 1-D, contiguous, 16-byte aligned and a multiple of 4 floats long')
    nc = start.numel()
    if start.dim() != 1 or not start.is_contiguous() or tuple(cap_or_n.shape) != (nc,) or not cap_or_n.is_contiguous():
        raise ValueError('audiogan_amd: start and %s must be contiguous vectors with one entry per clip' % second)
    return nc


@_timed(_work_named)
def clip_facts(bank, start, cap):
    """the packed store ``bank`` (fp32, clip c = bank[start[c] : start[c] + cap[c]], every start a multiple of 4 floats;
    ``start`` int64, ``cap`` int32) -> (n int32 [n_clips], peak fp32 [n_clips]): n = the index after the last sample that
    is not +-0 (a denormal and a NaN count), peak = max |x|, a NaN if the clip holds one, +inf for an infinite sample.
    Exact (ag_clip_facts: one launch, one workgroup per clip)."""
    nc = _clip_store(bank, start, cap, 'cap')
    n = torch.empty(nc, dtype=torch.int32, device=bank.device)
    peak = torch.empty(nc, dtype=torch.float32, device=bank.device)
    check(lib.ag_clip_facts(_p(bank), _p(start), _p(cap), _p(n), _p(peak), nc, _stream()), 'ag_clip_facts')
    return n, peak


@_timed(_work_named)
def clip_gather(bank, start, n, peak, ids, out, len_out=None, frame=0):
    """``ids`` int64 [B] on the device, every one a clip of the store (the CALLER's duty: ``dataset.ClipBatch`` checks them on
    the host); ``out`` fp32 [B, W], unit stride along W, any row pitch and alignment; ``len_out`` int64 [B] or None.
    out[b, t] = bank[start[c] + t] / peak[c] for t < min(n[c], W), c = ids[b], else 0 - the division correctly rounded, the
    bits of the host loader's float64 divide and float32 cast; len_out[b] = n[c] rounded up to ``frame`` (0: n[c]), not
    cropped to W (ag_clip_gather: one launch).  -> (out, len_out)"""
    nc = _clip_store(bank, start, n, 'n')
    _chk(peak, 'peak'); _chk(ids, 'ids', torch.int64); _chk(len_out, 'len_out', torch.int64)
    if tuple(peak.shape) != (nc,) or not peak.is_contiguous() or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError('audiogan_amd: peak must be a contiguous vector with one entry per clip, ids a contiguous vector')
    B = ids.numel()
    _chk(out, 'out')
    if out.dim() != 2 or out.size(0) != B or (out.size(1) > 1 and out.stride(1) != 1):
        raise ValueError('audiogan_amd: out must be [%d, W] with unit stride along W, got %r with strides %r'
                         % (B, tuple(out.shape), out.stride()))
    if len_out is not None and (tuple(len_out.shape) != (B,) or not len_out.is_contiguous()):
        raise ValueError('audiogan_amd: len_out must be a contiguous vector of %d entries' % B)
    W = out.size(1)
    ld = out.stride(0) if B > 1 else max(out.stride(0), W)
    check(lib.ag_clip_gather(_p(bank), _p(start), _p(n), _p(peak), _p(ids), B, _p(out), ld, W, _p(len_out), int(frame or 0),
                             _stream()), 'ag_clip_gather')
    return out, len_out


# ------------------------------------------------------------------------------------
# activity detection (audio.activity, ingest.build_store(trim / split)): frame power of ragged rows, runs of active frames
# ------------------------------------------------------------------------------------
FRAME_POWER_TILE_MAX = 256                                # frames: the largest tile of ag_frame_power
ACTIVITY_CHUNK = int(lib.ag_activity_chunk())             # frames ag_activity_segments walks at a time


def frame_power_ok(win, hop):
    """the library's rule for ag_frame_power and ag_activity_segments: 1 <= hop <= win <= 4096"""
    return bool(lib.ag_frame_power_ok(int(win), int(hop)))


def frame_power_tile(win, hop):
    """frames one workgroup of ag_frame_power takes at (win, hop): the most, up to 256, whose samples fit 64 KB of LDS"""
    return int(lib.ag_frame_power_tile(int(win), int(hop)))


@_timed(_work_named)
def frame_power(src, src_len, win, hop, dst=None, n_frames=None, in_start=0, f_start=0):
    """src [B, n_in] fp32 (unit stride along the samples, any row pitch and alignment): samples in_start .. in_start + len_b - 1
    of B signals, len_b = clamp(src_len[b], 0, n_in) (int64 [B] or None: n_in), zero elsewhere.  -> dst [B, n_frames] fp32:
    dst[b, j] = the mean of x^2 over samples f hop .. f hop + win - 1, f = f_start + j, in the fixed order of the header (block
    sums over gcd(win, hop) samples, then a chain per frame).  ``n_frames`` defaults to ceil(n_in / hop); ALL n_frames entries
    of every row are written.  A chunk of a signal (its two starts set) has the bits of the whole (ag_frame_power: one
    launch)."""
    _chk(src, 'src'); _chk(src_len, 'src_len', torch.int64)
    assert src.dim() == 2 and (src.size(1) <= 1 or src.stride(1) == 1), (tuple(src.shape), src.stride())
    B, n_in = src.size(0), src.size(1)
    pitch = src.stride(0) if B > 1 else max(src.stride(0), n_in)
    assert src_len is None or (src_len.is_contiguous() and src_len.numel() == B)
    if n_frames is None:
        n_frames = dst.size(1) if dst is not None else (n_in + int(hop) - 1) // int(hop)
    if dst is None:
        dst = torch.empty(B, n_frames, dtype=torch.float32, device=src.device)
    ldd = _rows(dst, 'dst', B, n_frames)
    check(lib.ag_frame_power(_p(src), pitch, _p(src_len), n_in, int(in_start), int(win), int(hop), _p(dst), ldd, int(f_start),
                             n_frames, B, _stream()), 'ag_frame_power')
    return dst


@_timed(_work_named)
def activity_segments(power, nf, lens, ratio, floor, min_gap, min_run, pad, win, hop, K=256, seg=None):
    """power [B, F] fp32 (unit stride along F, any row pitch), nf int32 [B] (<= F), lens int64 [B] -> (seg int64 [B, K, 2],
    count int32 [B], pmax fp32 [B]): the rule of the header - threshold max(pmax ratio, floor), gaps shorter than ``min_gap``
    frames closed, runs shorter than ``min_run`` frames dropped, ``pad`` frames added either side, overlapping or touching
    sample ranges merged.  count is the number of runs even above K; seg[b, k] is written for k < min(count, K) only (a ``seg``
    that is given keeps its other entries; a fresh one holds -1 there).  count = -1: a NaN or an infinity in the row
    (ag_activity_segments: one launch)."""
    _chk(power, 'power'); _chk(nf, 'nf', torch.int32); _chk(lens, 'lens', torch.int64); _chk(seg, 'seg', torch.int64)
    assert power.dim() == 2 and (power.size(1) <= 1 or power.stride(1) == 1), (tuple(power.shape), power.stride())
    B, F = power.size(0), power.size(1)
    pitch = power.stride(0) if B > 1 else max(power.stride(0), F)
    assert nf.is_contiguous() and nf.numel() == B and lens.is_contiguous() and lens.numel() == B
    K = int(K)
    if seg is None:
        seg = torch.full((B, max(K, 0), 2), -1, dtype=torch.int64, device=power.device)
    assert seg.is_contiguous() and tuple(seg.shape) == (B, K, 2), (tuple(seg.shape), (B, K, 2))
    count = torch.empty(B, dtype=torch.int32, device=power.device)
    pmax = torch.empty(B, dtype=torch.float32, device=power.device)
    check(lib.ag_activity_segments(_p(power), pitch, _p(nf), F, _p(lens), float(ratio), float(floor), int(min_gap), int(min_run),
                                   int(pad), int(win), int(hop), _p(seg), K, _p(count), _p(pmax), B, _stream()),
          'ag_activity_segments')
    return seg, count, pmax




# ------------------------------------------------------------------------------------
# sentence synthesis (synth.Voice.say_batch): the facts of ragged rows, the rows joined into sentences - no host read
# ------------------------------------------------------------------------------------
JOIN_MAX_SEGMENTS = int(lib.ag_join_max_segments())       # segments one sentence of ag_join_clips may hold
JOIN_MAX_FADE = 4096                                       # samples: the longest ramp of ag_join_clips
_RAMPS = {}


def join_ramp(F, device='cpu'):
    """fp32 [F] on ``device``: ramp[i] = sin^2(pi (i + 0.5) / (2 F)), evaluated in float64 and rounded once; strictly rising,
    ramp[i] + ramp[F - 1 - i] = 1 within 3e-8 - an overlap of exactly F samples is a constant-gain crossfade.  Cached per
    (F, device)."""
    F = int(F)
    if not 0 <= F <= JOIN_MAX_FADE:
        raise ValueError('audiogan_amd: a fade of %d samples: 0 .. %d' % (F, JOIN_MAX_FADE))
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if (F, 'cpu') not in _RAMPS:
        r = np.sin(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / (2.0 * max(F, 1))) ** 2
        _RAMPS[(F, 'cpu')] = torch.from_numpy(r.astype(np.float32))
    if (F, str(device)) not in _RAMPS:
        _RAMPS[(F, str(device))] = _RAMPS[(F, 'cpu')].to(device)
    return _RAMPS[(F, str(device))]


def _join_rows(wave, off, n):
    """the checks both launches share: fp32 rows of unit stride along the samples, one int32 offset and length per row
    -> (R, L_in, row pitch)"""
    _chk(wave, 'wave'); _chk(off, 'off', torch.int32); _chk(n, 'n', torch.int32)
    if wave.dim() != 2 or (wave.size(1) > 1 and wave.stride(1) != 1):
        raise ValueError('audiogan_amd: wave must be [R, L_in] with unit stride along L_in, got %r with strides %r'
                         % (tuple(wave.shape), wave.stride()))
    R, L_in = wave.size(0), wave.size(1)
    if tuple(off.shape) != (R,) or tuple(n.shape) != (R,) or not off.is_contiguous() or not n.is_contiguous():
        raise ValueError('audiogan_amd: off and n must be contiguous vectors with one entry per row of wave (%d)' % R)
    return R, L_in, wave.stride(0) if R > 1 else max(wave.stride(0), L_in)


# (neither launch is in the Profiler's timed set: that set is the training step's launches, which the bench's profile reports)
def join_facts(wave, off, n, target=0.0):
    """``wave`` fp32 [R, L_in] (unit stride along the samples, any row pitch), ``off`` / ``n`` int32 [R] on the device: row r's
    window is wave[r, off' : off' + n'], both clamped into the row.  -> (gain fp32 [R], bad int32 [R]): bad = 1 when the
    window holds a NaN or an infinity (gain 0 then), else gain = target / max |x| correctly rounded, 1 for a silent window
    or when ``target`` <= 0 (ag_join_facts: one launch, one workgroup per row, no host read)."""
    R, L_in, ld = _join_rows(wave, off, n)
    gain = torch.empty(R, dtype=torch.float32, device=wave.device)
    bad = torch.empty(R, dtype=torch.int32, device=wave.device)
    check(lib.ag_join_facts(_p(wave), ld, L_in, _p(off), _p(n), R, float(target), _p(gain), _p(bad), _stream()), 'ag_join_facts')
    return gain, bad


def join_clips(wave, off, n, gain, seg_row, join, sent_ptr, ramp, out, out_len=None, pause_max=0):
    """the windows of ``join_facts`` placed into sentences.  ``seg_row`` / ``join`` int32 [K], ``sent_ptr`` int32 [S + 1] on the
    device: sentence s owns segments sent_ptr[s] .. sent_ptr[s + 1] - 1 (at most JOIN_MAX_SEGMENTS: the CALLER's duty beyond
    K <= 1024 S), segment k is the window of row seg_row[k], join[k] >= 0 a pause of that many zero samples after it (at most
    ``pause_max``, a host integer), join[k] < 0 an overlap of min(-join[k], n_k / 2, n_{k+1} / 2) samples.  ``ramp`` fp32 [F]
    (``join_ramp``; F = 0: no fades) shapes the first and last min(F, n_k / 2) samples of every segment; ``gain`` fp32 [R]
    scales its row.  ``out`` fp32 [S, O_cap], unit stride along O_cap, any row pitch and alignment: EVERY entry is written
    (zeros in pauses and past a sentence's end); ``out_len`` int64 [S] receives each sentence's total, not cropped to O_cap.
    The arithmetic is the header's: products and sums rounded once each (ag_join_clips: one launch).  -> (out, out_len)"""
    R, L_in, ld = _join_rows(wave, off, n)
    _chk(gain, 'gain'); _chk(seg_row, 'seg_row', torch.int32); _chk(join, 'join', torch.int32)
    _chk(sent_ptr, 'sent_ptr', torch.int32); _chk(ramp, 'ramp'); _chk(out, 'out'); _chk(out_len, 'out_len', torch.int64)
    if tuple(gain.shape) != (R,) or not gain.is_contiguous():
        raise ValueError('audiogan_amd: gain must be a contiguous vector with one entry per row of wave (%d)' % R)
    if seg_row.dim() != 1 or tuple(join.shape) != tuple(seg_row.shape) or not seg_row.is_contiguous() or not join.is_contiguous():
        raise ValueError('audiogan_amd: seg_row and join must be contiguous vectors with one entry per segment')
    if sent_ptr.dim() != 1 or sent_ptr.numel() < 1 or not sent_ptr.is_contiguous():
        raise ValueError('audiogan_amd: sent_ptr must be a contiguous vector of S + 1 entries')
    if ramp.dim() != 1 or not ramp.is_contiguous():
        raise ValueError('audiogan_amd: ramp must be a contiguous vector (kernels.join_ramp)')
    K_, S = seg_row.numel(), sent_ptr.numel() - 1
    if out.dim() != 2 or out.size(0) != S or (out.size(1) > 1 and out.stride(1) != 1):
        raise ValueError('audiogan_amd: out must be [%d, O_cap] with unit stride along O_cap, got %r with strides %r'
                         % (S, tuple(out.shape), out.stride()))
    if out_len is None:
        out_len = torch.empty(S, dtype=torch.int64, device=out.device)
    if tuple(out_len.shape) != (S,) or not out_len.is_contiguous():
        raise ValueError('audiogan_amd: out_len must be a contiguous vector of %d entries' % S)
    O_cap = out.size(1)
    ldo = out.stride(0) if S > 1 else max(out.stride(0), O_cap)
    check(lib.ag_join_clips(_p(wave), ld, L_in, _p(off), _p(n), _p(gain), R, _p(seg_row), _p(join), _p(sent_ptr), K_, S,
                            int(pause_max), _p(ramp), ramp.numel(), _p(out), ldo, O_cap, _p(out_len), _stream()), 'ag_join_clips')
    return out, out_len


# ------------------------------------------------------------------------------------
# sample sheets (sheet.render, sheet.SheetWriter): a minibatch of ragged clips drawn as one image - no host read
# ------------------------------------------------------------------------------------
SHEET_TILE_COLUMNS = int(lib.ag_sheet_tile_columns())     # pixel columns one workgroup of ag_sheet_render takes
SHEET_HOP = 128                                            # samples per pixel column


def _rgb_word(c, name):
    r, g, b = (int(v) for v in c)
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError('audiogan_amd: the colour %s = %r: three values 0 .. 255' % (name, tuple(c)))
    return r | (g << 8) | (b << 16)


# (not in the Profiler's timed set: that set is the training step's launches, which the bench's profile reports)
def sheet_render(wave, lens, power, nframes, thresholds, cmap, img, cols, Hw, gutter, bg=(32, 32, 32), paper=(255, 255, 255),
                 ink=(0, 0, 0)):
    """``wave`` fp32 [B, L] (unit stride along the samples, any row pitch), ``lens`` int64 [B] on the device or None (L),
    ``power`` fp32 [B, F, 129] and ``nframes`` int32 [B] as ``melcep_frames`` leaves them, ``thresholds`` fp32 [256]
    (``sheet.thresholds``), ``cmap`` uint8 [256, 3], ``img`` uint8 [H, W, 3] of exactly ``sheet.sheet_geometry``'s size, at any
    byte alignment: tile b at grid cell (b div cols, b mod cols), ``Hw`` rows of waveform envelope over 129 rows of spectrogram
    (bin 0 at the bottom), one pixel column per 128 samples, ``gutter`` pixels of ``bg`` around every tile.  The rules of both
    halves are the header's, exact: EVERY pixel of ``img`` is written, nothing is read to the host (ag_sheet_render: one
    launch).  -> img"""
    if wave.dim() != 2 or power.dim() != 3 or img.dim() != 3:
        raise ValueError('audiogan_amd: wave must be [B, L], power [B, F, 129] and img [H, W, 3], got %r, %r and %r'
                         % (tuple(wave.shape), tuple(power.shape), tuple(img.shape)))
    (B, L), F, (H, W) = wave.shape, power.shape[1], img.shape[:2]
    ld = _check_table([(wave, 'wave', (B, L), _PITCHED), (lens, 'lens', (B,), torch.int64),
                       (power, 'power', (B, F, LTAS_BINS)), (nframes, 'nframes', (B,), torch.int32),
                       (thresholds, 'thresholds', (256,)), (cmap, 'cmap', (256, 3), torch.uint8),
                       (img, 'img', (H, W, 3), torch.uint8)])
    check(lib.ag_sheet_render(_p(wave), ld['wave'], _p(lens), L, _p(power), _p(nframes), F, B, _p(thresholds), _p(cmap),
                              _rgb_word(bg, 'bg'), _rgb_word(paper, 'paper'), _rgb_word(ink, 'ink'), int(cols), int(Hw),
                              int(gutter), _p(img), H, W, _stream()), 'ag_sheet_render')
    return img

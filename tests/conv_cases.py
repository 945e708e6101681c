"""Shared pieces of the conv dispatch fuzz (test_conv_fuzz.py on the GPU, test_conv_fuzz_host.py against the CPU model)
--  TEST INFRASTRUCTURE, no test functions.

  conv_plan() / wgrad_plan() / o1_plan() / sum_plan() / leaky_plan()
                        a restatement, on sizes, strides and alignment alone, of the dispatch of conv_engine.hip
                        (ag_conv1d_engine), conv_engine_impl.h (launch_cfg / launch_bf16 / launch_bf16_nw), conv_c1.hip and
                        conv_grad.hip.  Each returns the kernel name as ag_last_kernel reports it (main launch only), the
                        tail launch that follows it, the runtime form (generic | pipe | solo | solo+dma; bf16: NW, nbuf), the
                        chunk count and whether the last chunk is ragged, `aligned`, `xvec`; for the weight gradient TC,
                        nchunk, gz and the workspace it asks for; for the c1 / o1 / channel-sum kernels which kernel and how
                        many slabs.  THE RUNTIME FLAGS CANNOT BE READ BACK FROM THE LIBRARY: they are restated conditions,
                        cross-checked on the GPU only through the kernel name (asserted equal for every case) and through
                        ag_conv1d_wgrad_ws_numel (asserted equal for every weight-gradient case).  The o1, channel-sum and
                        leaky kernels report no name; their forms are restated conditions only.
  engine_cases() / wgrad_cases() / small_cases()
                        a pinned list (one case per class the coverage assertions name) followed by seeded random cases;
                        the first 40 random engine / weight-gradient cases are the 40 seeded shapes the earlier version of
                        test_conv_fuzz.py drew (forward with its epilogue options, backward-data, backward-weight).  Pinned
                        shapes are the smallest that reach their branch: wide tiles are reached with a large batch and thin
                        layers, none is a workload size.  NOT REACHED: the full tile's solo limit (C taps = 512)
                        in fp32 mode - 512 workgroups over that reduction are 1.1e9 multiply-adds; bf16 mode reaches both sides
                        through its fall-back -, the 31-bit `efast` = false branch of the epilogue
                        and the >= 2^31-byte refusals of the pipelined / bf16 staging (a 2 GiB span each), the bf16
                        weight-gradient kernel's 2^30 offset limits, and LDS sizes beyond 160 KiB.
  make_inputs()         the operands of one case for one PASS:
                          EXACT  operands, bias, residual, prior output and dw0 are integers in [-3, 3], slope 0.5.  With
                                 9 x (reduction length) < 2^24 (host test: asserted for every case; C K for the engine, B Lsh
                                 for the weight gradient, B L for the sums) every fp32 order of summation is exact and bf16
                                 holds the operands, so every output equals the float64 reference BIT FOR BIT in both
                                 precision modes: a tap, phase, halo or tail column that is dropped, doubled or shifted by
                                 one cannot hide.
                          REAL   randn operands, weights scaled by (C K)^-1/2 (weight gradient: operands scaled so that dw
                                 is of order 1), bias / residual / prior output of the product's size, slope LEAKY_SLOPE.
  reference()           float64, from the contract in include/audiogan_hip.h, written with F.conv1d / F.conv_transpose1d in
                        double; in bf16 mode on operands rounded to bf16 (nearest even), as the mode defines.
  run_*()               place every tensor as the case says; every output is a window in a sentinel-filled frame (channels
                        above and below, pitch padding left and right, a batch row before and after; a contiguous output:
                        guard floats before and after), NaN-filled when the call does not accumulate.  Returns the
                        window(s), the kernel name and whether the frame is bit-for-bit untouched.
  check()               EXACT: torch.equal with the reference, no NaN, frame untouched.  REAL: the bound rule of DESIGN.md
                        section 2 - floor = the error of the fp32 CPU model (tests/kernel_model.py) against the float64
                        reference as a fraction of the reference's largest magnitude, not below 2^-24; bound = 16 x floor,
                        never above the declared 1e-4 of the output scale.
"""
import collections

import torch
import torch.nn.functional as F

from tests import kernel_model as KM

ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_LEAKY_GATE = 0, 1, 2, 3
LEAKY_SLOPE = 0.01

EXACT = dict(name='exact', slope=0.5)
REAL = dict(name='real', slope=LEAKY_SLOPE)

SENTINEL = -12345.0
GUARD = 64                 # floats before and after every buffer (keeps 16-byte alignment)

MAC_MAX = 4e8              # per case
MAC_SUM_MAX = 2e10         # per GPU test function
FRAME_MAX = 64e6           # bytes per frame

# bound rule (as the recurrent fuzz declares it)
MARGIN = 16.0
MARGIN_MAX = 64.0
FLOOR_MIN = 2.0 ** -24
CEIL = 1e-4
# (kernel form, output) -> a margin above 16, at most MARGIN_MAX, each with its reason.  None is needed: see
# profiles/conv_fuzz.txt for the measured error / floor per form.
MARGINS = {}

MAX_TAPS = 32
CONV_SOLO_K = 512
CB_NX = 2
WB_FS, WB_FL = 8, 5
O1_MAXK = 9


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def margin_of(form, output=''):
    m = MARGINS.get((form, output), MARGIN)
    assert MARGIN <= m <= MARGIN_MAX
    return m


def bound(margin, floor):
    return min(margin * max(floor, FLOOR_MIN), CEIL)


# ---------------------------------------------------------------------------------------------------------------------
# views: how a [B, C, L] tensor sits in memory
#   'c'  contiguous (guard floats around)          'a'  channel block, aligned: pitch % 4 == 0, column offset 4
#   'o'  channel block, odd pitch, column offset 3 'h'  pitch % 4 == 2, column offset 4 (base aligned when C is even)
#   'm'  pitch % 4 == 0, column offset 5 (base + 1 float)
#   'l'  the slab of the earlier fuzz: [B, C + 2, L + 12][:, 1:C + 1, 4:L + 4] (aligned iff L % 4 == 0)
# ---------------------------------------------------------------------------------------------------------------------
def geom(view, C, L):
    """dict(bpad, ca, cb, off, pitch): batch rows around, channels above / below, column offset, row pitch"""
    if view == 'c':
        return dict(bpad=0, ca=0, cb=0, off=0, pitch=L)
    if view == 'a':
        return dict(bpad=1, ca=1, cb=2, off=4, pitch=roundup(L + 8, 4))
    if view == 'o':
        return dict(bpad=1, ca=1, cb=2, off=3, pitch=(L + 7) | 1)
    if view == 'h':
        return dict(bpad=1, ca=1, cb=2, off=4, pitch=roundup(L + 8, 4) + 2)
    if view == 'm':
        return dict(bpad=1, ca=1, cb=2, off=5, pitch=roundup(L + 9, 4))
    assert view == 'l', view
    return dict(bpad=0, ca=1, cb=1, off=4, pitch=L + 12)


def strides(view, C, L):
    """(base offset in floats from a 16-byte aligned address, batch stride, channel stride)"""
    g = geom(view, C, L)
    cs = g['pitch']
    bs = (C + g['ca'] + g['cb']) * cs
    return GUARD + g['bpad'] * bs + g['ca'] * cs + g['off'], bs, cs


def vec_ok(view, C, L):
    """16-byte aligned base, batch and channel strides % 4 == 0"""
    base, bs, cs = strides(view, C, L)
    return base % 4 == 0 and bs % 4 == 0 and cs % 4 == 0


class Frame(object):
    """a [B, C, L] window (view form `view`) inside a sentinel-filled buffer"""

    def __init__(self, B, C, L, view, device, fill, sentinel=SENTINEL):
        g = geom(view, C, L)
        rows, pitch = C + g['ca'] + g['cb'], g['pitch']
        n = (B + 2 * g['bpad']) * rows * pitch
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=torch.float32, device=device)
        box = self.buf[GUARD:GUARD + n].view(B + 2 * g['bpad'], rows, pitch)
        self.sl = (slice(g['bpad'], g['bpad'] + B), slice(g['ca'], g['ca'] + C), slice(g['off'], g['off'] + L))
        self.box, self.win = box, box[self.sl]
        if fill is not None:
            self.win.copy_(fill)
        self.before = self.buf.cpu().clone()
        assert self.buf.numel() * 4 <= FRAME_MAX + 8 * GUARD, 'frame too large'
        assert (self.win.stride(0), self.win.stride(1)) == strides(view, C, L)[1:] or B == 1 or C == 1

    def untouched(self):
        after, before = self.buf.cpu().clone(), self.before.clone()
        n = after.numel() - 2 * GUARD
        for t in (after, before):
            t[GUARD:GUARD + n].view(self.box.shape)[self.sl] = 0
        return torch.equal(after.view(torch.int32), before.view(torch.int32))

    def window(self):
        return self.win.cpu().clone()


class FlatFrame(object):
    """a contiguous tensor of `shape` between guard floats (`dtype`: fp32, or bf16 / an integer type for the outputs of the
    pointwise fuzz that are stored so)"""

    def __init__(self, shape, device, fill, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.n, self.lo = n, GUARD
        self.bits = {4: torch.int32, 2: torch.int16, 8: torch.int64}[torch.empty(0, dtype=dtype).element_size()]
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
        self.win = self.buf[self.lo:self.lo + n].view(*shape)
        self.win.copy_(fill)
        self.before = self.buf.cpu().clone()

    def untouched(self):
        after = self.buf.cpu()
        return torch.equal(after[:self.lo].view(self.bits), self.before[:self.lo].view(self.bits)) and \
            torch.equal(after[self.lo + self.n:].view(self.bits), self.before[self.lo + self.n:].view(self.bits))

    def window(self):
        return self.win.cpu().clone()


class StridedFrame(object):
    """a window of `shape` and any `strides` (in floats, from `off` floats behind the front guard) inside a sentinel-filled
    buffer: a transposed view, a column of a wider tensor, a view with no unit stride"""

    def __init__(self, shape, strides, off, device, fill, sentinel=SENTINEL):
        span = 1 + sum((n - 1) * st for n, st in zip(shape, strides))
        self.buf = torch.full((off + span + 2 * GUARD,), sentinel, dtype=torch.float32, device=device)
        self.geo = (tuple(shape), tuple(strides), GUARD + off)
        self.win = self.buf.as_strided(*self.geo)
        if fill is not None:
            self.win.copy_(fill)
        self.before = self.buf.cpu().clone()

    def untouched(self):
        after, before = self.buf.cpu().clone(), self.before.clone()
        for t in (after, before):
            t.as_strided(*self.geo).zero_()
        return torch.equal(after.view(torch.int32), before.view(torch.int32))

    def window(self):
        return self.win.cpu().clone()


def place(t, view, device):
    """an input tensor in view form `view` (its surroundings hold 99)"""
    B, C, L = t.shape
    return Frame(B, C, L, view, device, t, sentinel=99.0).win


# ---------------------------------------------------------------------------------------------------------------------
# the engine: cases and the dispatch restated
# ---------------------------------------------------------------------------------------------------------------------
# mode 0: y[b,o,t] = sum W[o,c,k] x[b,c,s t + k - p];  mode 1: y[b,o,s t + k - p] += W[c,o,k] x[b,c,t]
EC = collections.namedtuple('EC', 'mode B C O K s p Lin Lout o')


def eopts(bias=0, res=0, act=ACT_NONE, lens=0, acc=0, xv='c', yv='a', rv=None, wp0=0):
    """lens: 0 none, 1 random in [1, Lout], 2 holding 0, 1 and Lout (B >= 3);  xv / yv / rv: view forms of x, y and res;
    wp0: mode 1 - the scatter layout was prepared for padding 0 and the call says so (wp_pad = 0)"""
    if act == ACT_LEAKY_GATE:
        res = 1                    # the gate's saved activation travels in `res`
    return dict(bias=bias, res=res, act=act, lens=lens, acc=acc, xv=xv, yv=yv, rv=rv or yv, wp0=wp0)


def out_len(mode, K, s, p, Lin, extra=0):
    return (Lin + 2 * p - K) // s + 1 if mode == 0 else (Lin - 1) * s - 2 * p + K + extra


def ecase(mode, B, C, O, K, s, p, Lin, extra=0, **kw):
    """extra (mode 1): output positions beyond the last scattered one (a conv's backward-data whose input length left a
    remainder; ConvTranspose1d's output_padding)"""
    return EC(mode, B, C, O, K, s, p, Lin, out_len(mode, K, s, p, Lin, extra), eopts(**kw))


def engine_macs(c):
    return c.B * c.O * c.Lout * c.C * c.K if c.mode == 0 else c.B * c.C * c.Lin * c.O * c.K


def scatter_aligned(c):
    return c.mode == 1 and not c.o['wp0'] and KM._scatter_aligned(c.K, c.s, c.p)


TILES = {'1214': (1, 2, 1, 4), '2114': (2, 1, 1, 4), '1122': (1, 1, 2, 2), '2122': (2, 1, 2, 2), '2222': (2, 2, 2, 2),
         '1141': (1, 1, 4, 1)}
TAP_KEYS = (1708, 904, 702, 301, 1608, 804, 200, 300, 400)


def _launch_bf16(c, cfg, taps, sp, Cpad, xvec):
    """launch_bf16 / launch_bf16_nw: None = the shape does not fit (caller keeps the fp32-MFMA kernel on rounded operands)"""
    TO, TTL, WO, WT = cfg
    OT, TT = 32 * TO * WO, 32 * TTL * WT
    if not xvec or c.Lin % 4 != 0:
        return None
    dmax = (c.K - 1) // c.s if c.mode == 0 else taps - 1
    ncols = TT + dmax
    chs = sp * ncols
    groups = cdiv(Cpad, 16)

    def nw_form(NW):
        per_g = (2 * chs + taps * 2 * OT) * 16
        ng = max(1, min(4, ((74 if NW > 8 else 36) * 1024) // per_g, groups))
        nq = (sp * ncols + 6) // 4 + 1
        while ng > 1 and (ng * taps * 2 * OT > NW * 256 or ng * 2 * nq > CB_NX * 256):
            ng -= 1
        if taps * 2 * OT > NW * 256 or 2 * nq > CB_NX * 256:
            return None
        nbuf = 1 if ng >= groups else 2
        if nbuf * ng * per_g + OT * 4 > 160 * 1024:
            return None
        chunks = cdiv(groups, ng)
        return dict(kernel='conv_engine_bf16_kernel<%d,%d,%d,%d,%d>' % (TO, TTL, WO, WT, NW), form='bf16', nw=NW, nbuf=nbuf,
                    cc=16 * ng, chunks=chunks, last=16 * (groups - (chunks - 1) * ng))
    if OT >= 128 and groups * taps >= 32:
        r = nw_form(16)
        if r is not None:
            return r
    return nw_form(8)


def _launch_cfg(c, tile, n_cnt, rb, xvec):
    """launch_cfg<TO,TTL,WO,WT> of conv_engine_impl.h for `n_cnt` columns"""
    cfg = TILES[tile]
    TO, TTL, WO, WT = cfg
    OT, TT = 32 * TO * WO, 32 * TTL * WT
    taps, sp = (c.K, c.s) if c.mode == 0 else (cdiv(c.K, c.s), 1)
    Mrows = c.O if c.mode == 0 else c.O * c.s
    Cpad, Mpad = roundup(c.C, 2), roundup(Mrows, 32)
    grid = (cdiv(n_cnt, TT), cdiv(Mrows, OT), c.B)
    if rb and c.C >= 16:
        r = _launch_bf16(c, cfg, taps, sp, Cpad, xvec)
        if r is not None:
            return dict(r, tile=(OT, TT), grid=grid, n_cnt=n_cnt)
    dmax = (c.K - 1) // c.s if c.mode == 0 else taps - 1
    ncols = TT + dmax
    rl = ncols
    if sp > 1 and sp <= 32 and sp & (sp - 1) == 0:
        rl = ncols + (32 // sp - ncols) % 32
    if sp & 1 and rl & 1:
        rl += 1
    chs = sp * rl
    per_c = (chs + taps * OT) * 4

    def generic_cc():
        return min(max((36 * 1024 // per_c) & ~1, 2), 32, Cpad)
    cc, form = generic_cc(), 'generic'
    if xvec and c.Lin % 4 == 0 and c.Lin >= 4:
        nq = (sp * ncols + 6) // 4 + 1
        FXH, FWH = (7, 3) if OT <= 32 else (4, 8)
        cf = cc
        while cf > 2 and (cf * nq > FXH * 256 or cf * taps * (OT // 4) > FWH * 256):
            cf -= 2
        if cf * nq <= FXH * 256 and cf * taps * (OT // 4) <= FWH * 256 and cf < Cpad:
            cc, form = cf, 'pipe'
    per_cs = per_c
    if OT == 128 and TT in (128, 64):
        if c.mode == 1 and Cpad * taps <= (CONV_SOLO_K // 4 if TT == 64 else CONV_SOLO_K):
            if not rb and xvec and c.Lin % 4 == 0 and Cpad % 16 == 0 and Mpad % 4 == 0:
                form = 'solo+dma'
                per_cs = (roundup(4 * ((ncols + 6) // 4), 16) + taps * OT) * 4
                cc = 32 if (Cpad % 32 == 0 and 32 * per_cs <= 40 * 1024) else 16
            else:
                form, cc = 'solo', generic_cc()
    lds = (1 if form.startswith('solo') else 2) * cc * per_cs + OT * 4
    assert lds <= 160 * 1024, 'the tile needs more LDS than the engine takes'
    if tile in ('1122', '1141'):
        key = -1                                   # the tail tiles have no tap specialisations
    else:
        key = taps * 100 + c.s if c.mode == 0 else taps * 100
    T, S0 = (key // 100, key % 100) if key in TAP_KEYS else (0, 0)
    chunks = cdiv(Cpad, cc)
    return dict(kernel='conv_engine_kernel<%d,%d,%d,%d,%d,%d>' % (TO, TTL, WO, WT, T, S0), form=form, nw=0, nbuf=0, cc=cc,
                chunks=chunks, last=Cpad - (chunks - 1) * cc, tile=(OT, TT), grid=grid, n_cnt=n_cnt,
                key=key if key in TAP_KEYS else 0)


def conv_plan(prec, c):
    """what ag_conv1d_engine launches for case `c` in precision mode `prec` ('f32' / 'bf16')"""
    rb, o = prec == 'bf16', c.o
    xvec = vec_ok(o['xv'], c.C, c.Lin)
    aligned = scatter_aligned(c)
    base = dict(aligned=aligned, xvec=xvec, tail=None, form='c1', nw=0, nbuf=0, chunks=1, last=0, key=0)
    if c.mode == 0:
        taps, Mrows, n_lo, n_cnt = c.K, c.O, 0, c.Lout
    else:
        taps, Mrows = cdiv(c.K, c.s), c.O * c.s
        if aligned:
            n_lo, n_cnt = cdiv(c.p, c.s), cdiv(c.Lout, c.s)
        else:
            n_lo = c.p // c.s
            n_cnt = (c.Lout - 1 + c.p) // c.s - n_lo + 1
    base.update(n_lo=n_lo, n_cnt=n_cnt, taps=taps, Mrows=Mrows)
    c1 = c.s == 2 and c.K == 7
    if c.mode == 0 and c.C == 1 and not o['res'] and not o['acc'] and c1 and o['act'] != ACT_LEAKY_GATE and \
            vec_ok(o['yv'], c.O, c.Lout):
        return dict(base, kernel='conv_c1_fwd_kernel<2,7,4>', slabs=cdiv(c.Lout, 1024))
    if c.mode == 1 and c.O == 1 and not (o['res'] or o['bias'] or o['lens']) and o['act'] == ACT_NONE and c1 and c.C <= 512:
        return dict(base, kernel='conv_c1_bwdx_kernel<2,7,4>', slabs=cdiv(c.Lin + 3, 1024))
    assert taps <= MAX_TAPS
    Cpad = roundup(c.C, 2)

    def one(tile, cols=n_cnt):
        return dict(base, **_launch_cfg(c, tile, cols, rb, xvec))

    def two(main, tail_tile, main_cols, tail):
        m = one(main, main_cols)
        m['tail'] = dict(_launch_cfg(c, tail_tile, tail, rb, xvec), n_lo=n_lo + main_cols)
        return m
    if Mrows <= 32:
        return one('1214')
    tail0 = n_cnt % 128
    tail = tail0 if (n_cnt - tail0) // 128 < 8 else 0
    main_cols = n_cnt - tail
    if Mrows <= 64:
        if 0 < tail <= 32 and main_cols > 0:
            return two('2114', '1122', main_cols, tail)
        return one('2114')
    if n_cnt <= 64:
        return one('2122')
    if c.mode == 1 and taps == 2 and not rb:
        return one('2122')
    bfp = rb and cdiv(Cpad, 16) * taps >= 32
    if not bfp and cdiv(n_cnt, 128) * cdiv(Mrows, 128) * c.B < 512:
        return one('2122')
    if 0 < tail <= 32 and main_cols > 0:
        half = not bfp and (main_cols // 128) * cdiv(Mrows, 128) * c.B < 512
        return two('2122' if half else '2222', '1141', main_cols, tail)
    return one('2222')


def plan_class(pl, c):
    """(form, chunk class, tail tile, aligned scatter, xvec) - what the coverage lists count"""
    chunks = 'one' if pl['chunks'] == 1 else ('last2' if pl['last'] == 2 else 'several')
    return (pl['form'] + (str(pl['nw']) + 'x' + str(pl['nbuf']) if pl['form'] == 'bf16' else ''), chunks,
            pl['tail']['tile'] if pl['tail'] else None, bool(pl['aligned']), bool(pl['xvec']))


N_, L_, G_ = ACT_NONE, ACT_LEAKY, ACT_LEAKY_GATE

# One case per class.  The comment names what the case is there for; tests/test_conv_fuzz_host.py asserts each claim on the
# plan, so a change of the dispatch that moves a case off its branch fails there first.
PINNED_ENGINE = [
    # --- tiles (fp32 mode) ---------------------------------------------------------------------------------------
    ('128x128', ecase(0, 512, 6, 96, 3, 1, 1, 96, bias=1, act=L_)),
    ('128x128+tail', ecase(0, 512, 6, 96, 3, 1, 1, 140, bias=1, res=1, acc=1, yv='o')),
    ('half+tail', ecase(0, 256, 6, 96, 3, 1, 1, 140, lens=2, act=L_)),
    ('128x128 mode1', ecase(1, 512, 6, 24, 12, 4, 4, 128, bias=1)),                 # Mrows 96, taps 3, solo
    ('64x128+tail', ecase(1, 2, 16, 16, 8, 4, 1, 130, bias=1, res=1)),              # Mrows 64, aligned scatter, tail
    ('64x128+tail acc', ecase(1, 2, 16, 16, 8, 4, 1, 130, acc=1, lens=1)),
    ('64x128', ecase(0, 2, 16, 64, 3, 1, 1, 200, act=L_, res=1)),
    ('32x256', ecase(0, 2, 17, 32, 5, 1, 2, 300, bias=1, lens=1)),
    ('128x64 n<=64', ecase(0, 2, 16, 65, 3, 1, 1, 64, bias=1)),
    ('128x64 taps2', ecase(1, 2, 32, 16, 16, 8, 4, 128, bias=1, act=L_)),           # the generator's k = 2s deconv
    ('tail1', ecase(0, 256, 6, 96, 3, 1, 1, 129, acc=1)),
    ('tail32', ecase(0, 256, 6, 96, 3, 1, 1, 160, bias=1)),
    ('tail33', ecase(0, 256, 6, 96, 3, 1, 1, 161, bias=1)),                         # no tail launch: 33 > 32
    ('main0', ecase(0, 2, 16, 64, 3, 1, 1, 20, bias=1)),                            # main_cols = 0: n_cnt = 20 < 128
    ('8 column tiles', ecase(1, 1, 16, 16, 8, 4, 1, 1026, bias=1)),                 # n_cnt = 1027: 8 tiles, no tail
    ('7 column tiles', ecase(1, 1, 16, 16, 8, 4, 1, 898, bias=1)),                  # n_cnt = 899: 7 tiles + tail 3
    # --- n_cnt around 64 and 128 ---------------------------------------------------------------------------------
    ('n65', ecase(0, 2, 16, 65, 3, 1, 1, 65)),
    ('n63', ecase(0, 2, 16, 65, 3, 1, 1, 63)),
    ('n127', ecase(0, 2, 16, 65, 3, 1, 1, 127, xv='a')),
    ('n129', ecase(0, 2, 16, 65, 3, 1, 1, 129, xv='a')),
    # --- modes: forward and the other kind's backward-data, out_pad ------------------------------------------------
    ('m1 bwd of conv, extra', ecase(1, 3, 32, 16, 9, 4, 4, 64, extra=3, res=1, act=G_, lens=2)),
    ('m1 out_pad', ecase(1, 3, 24, 33, 7, 3, 2, 50, extra=2, bias=1)),
    ('m0 bwd of convT', ecase(0, 2, 33, 24, 8, 4, 2, 258, acc=1)),
    # --- tap keys not reached above, strides 3 and 5, 32 taps, K = 1 ----------------------------------------------
    ('key1708', ecase(0, 2, 2, 128, 17, 8, 8, 1024, bias=1, act=L_)),
    ('key904', ecase(0, 2, 16, 64, 9, 4, 4, 512, bias=1)),
    ('key702', ecase(0, 2, 16, 32, 7, 2, 3, 256, bias=1, act=L_)),
    ('key1608', ecase(0, 2, 16, 64, 16, 8, 4, 1024)),
    ('key804', ecase(0, 2, 16, 64, 8, 4, 2, 512, acc=1)),
    ('key400', ecase(1, 2, 32, 16, 7, 2, 3, 128, res=1, act=G_)),
    ('key300 k17s8', ecase(1, 2, 128, 2, 17, 8, 8, 128, acc=1)),
    ('stride3', ecase(0, 2, 16, 64, 7, 3, 2, 301, bias=1)),
    ('stride5', ecase(1, 2, 16, 16, 11, 5, 3, 60, bias=1, lens=1)),
    ('taps32', ecase(0, 1, 4, 33, 32, 2, 15, 200, bias=1)),
    ('K1', ecase(0, 3, 40, 33, 1, 1, 0, 100, bias=1, act=L_)),
    ('K1 m1', ecase(1, 3, 40, 33, 1, 1, 0, 100, acc=1)),
    # --- staging forms: generic / pipe / solo / solo+dma, chunks ---------------------------------------------------
    ('pipe several', ecase(0, 2, 64, 128, 3, 1, 1, 256, bias=1)),
    ('pipe last2', ecase(0, 2, 42, 128, 3, 1, 1, 256, bias=1, res=1)),               # chunks of 20, 20, 2
    ('pipe last2 odd C', ecase(0, 2, 41, 128, 3, 1, 1, 256, acc=1)),                 # ... the last one half pad row
    ('generic one', ecase(0, 2, 16, 128, 3, 1, 1, 250)),
    ('generic several', ecase(0, 2, 64, 128, 3, 1, 1, 250, bias=1)),
    ('generic last2', ecase(0, 2, 41, 128, 3, 1, 1, 250, xv='o')),
    ('solo Lin3', ecase(1, 2, 17, 33, 8, 4, 2, 3, bias=1)),
    ('solo Lin1', ecase(1, 2, 17, 33, 8, 4, 2, 1, bias=1, acc=1)),
    ('generic Lin3 m0', ecase(0, 2, 17, 33, 3, 1, 1, 3, bias=1, act=L_)),
    ('generic Lin1 m0', ecase(0, 2, 17, 33, 3, 1, 1, 1, bias=1)),
    ('solo half <=128', ecase(1, 2, 30, 16, 16, 8, 4, 128, bias=1)),                # Cpad taps = 60
    ('solo half 128', ecase(1, 2, 64, 16, 16, 8, 4, 128, xv='o')),                  # Cpad taps = 128: solo, generic staging
    ('solo half >128', ecase(1, 2, 66, 16, 16, 8, 4, 128)),                         # 132: 8-wave form
    ('solo+dma cc16', ecase(1, 2, 48, 16, 16, 8, 4, 128, bias=1, res=1)),
    ('solo+dma cc32', ecase(1, 2, 64, 40, 4, 4, 0, 128, bias=1, act=L_)),           # one tap: 32 channels fit 40 KiB
    ('solo+dma full', ecase(1, 512, 16, 24, 12, 4, 4, 128, bias=1, acc=1)),         # taps 3: key 300 on the 128 x 128 tile
    ('full solo last2', ecase(1, 512, 33, 17, 4, 4, 0, 68, bias=1)),                 # 128 x 128, chunks of 32 + 2 (pad row)
    ('full solo last2 k12', ecase(1, 512, 18, 17, 12, 4, 4, 68, acc=1)),            # ... 16 + 2 on the 3-tap specialisation
    ('full solo several', ecase(1, 512, 36, 17, 4, 4, 0, 68, xv='o', res=1)),       # 32 + 4
    ('full solo+dma several', ecase(1, 512, 48, 17, 4, 4, 0, 68, bias=1, act=L_)),  # 3 chunks of 16
    ('bf16 full solo 512', ecase(1, 2, 128, 17, 16, 4, 4, 66, bias=1)),             # bf16 mode: Lin % 4 -> fp32 kernel, full tile
    ('bf16 full 8-wave 520', ecase(1, 2, 130, 17, 16, 4, 4, 66, bias=1)),           # ... just above the solo limit
    ('solo several last2', ecase(1, 2, 58, 40, 16, 8, 4, 128, xv='o')),             # chunks of 28, 28, 2
    ('solo last2 odd C', ecase(1, 2, 57, 40, 16, 8, 4, 128)),
    # --- alignment of x --------------------------------------------------------------------------------------------
    ('x misaligned', ecase(0, 2, 24, 40, 5, 2, 2, 256, xv='m', bias=1)),
    ('x odd pitch', ecase(1, 2, 24, 40, 8, 4, 2, 64, xv='o', bias=1)),
    ('x aligned pitched', ecase(0, 2, 24, 40, 5, 2, 2, 256, xv='a', bias=1)),
    # --- bf16 kernel classes (fp32 mode runs them on the fp32 kernels) ---------------------------------------------
    ('bf16 C16', ecase(0, 2, 16, 64, 7, 2, 3, 256, bias=1, xv='a')),
    ('bf16 C17', ecase(0, 2, 17, 64, 7, 2, 3, 256, bias=1)),
    ('bf16 C48 nbuf1', ecase(1, 2, 48, 40, 8, 4, 2, 128, acc=1)),
    ('bf16 nbuf2', ecase(0, 2, 130, 128, 3, 1, 1, 256, bias=1)),
    ('bf16 NW16', ecase(0, 16, 192, 128, 3, 1, 1, 256, bias=1, res=1, act=L_)),     # 12 groups x 3 taps >= 32
    ('bf16 NW16 + tail', ecase(0, 4, 192, 128, 3, 1, 1, 140, lens=2)),             # bfp: full tile whatever the grid
    ('bf16 C<16', ecase(0, 2, 12, 64, 7, 2, 3, 256, bias=1)),
    ('bf16 x unaligned', ecase(0, 2, 32, 64, 7, 2, 3, 256, xv='m')),
    ('bf16 Lin%4', ecase(0, 2, 32, 64, 7, 2, 3, 254, bias=1)),
    # --- scatter layouts --------------------------------------------------------------------------------------------
    ('scatter s4 aligned', ecase(1, 3, 16, 40, 9, 4, 3, 128, bias=1, lens=2)),      # 16-byte window rotated by pad % s
    ('scatter s8 aligned', ecase(1, 3, 16, 24, 17, 8, 4, 64, bias=1, lens=2)),      # pad % s a multiple of 4: plain
    ('scatter s2 aligned', ecase(1, 2, 16, 40, 7, 2, 3, 128, bias=1, res=1)),
    ('scatter pad%s==0', ecase(1, 2, 16, 40, 8, 4, 4, 128, bias=1)),
    ('scatter extra slot', ecase(1, 2, 16, 40, 8, 4, 2, 128, bias=1)),              # k = 2 s: the shifted phases need a third slot
    ('scatter wp_pad 0', ecase(1, 2, 16, 40, 8, 4, 2, 128, bias=1, wp0=1)),
    # --- single-channel forward / backward-data --------------------------------------------------------------------
    ('c1 fwd', ecase(0, 3, 1, 16, 7, 2, 3, 2050, bias=1, act=L_, lens=2)),          # Lout 1025: two blocks
    ('c1 fwd 1024', ecase(0, 2, 1, 18, 7, 2, 3, 2048, bias=1)),
    ('c1 fwd declined res', ecase(0, 2, 1, 16, 7, 2, 3, 300, res=1)),
    ('c1 fwd declined acc', ecase(0, 2, 1, 16, 7, 2, 3, 300, acc=1)),
    ('c1 fwd declined gate', ecase(0, 2, 1, 16, 7, 2, 3, 300, act=G_)),
    ('c1 fwd declined y base', ecase(0, 2, 1, 16, 7, 2, 3, 300, yv='m')),
    ('c1 fwd declined y pitch', ecase(0, 2, 1, 16, 7, 2, 3, 300, yv='h')),
    ('c1 bwdx', ecase(1, 3, 16, 1, 7, 2, 3, 1025, extra=1)),
    ('c1 bwdx acc', ecase(1, 2, 16, 1, 7, 2, 3, 1024, acc=1)),
    ('c1 bwdx unaligned layout', ecase(1, 2, 16, 1, 7, 2, 3, 300, wp0=1)),
    ('c1 bwdx unaligned acc', ecase(1, 2, 17, 1, 7, 2, 2, 300, acc=1)),
    ('c1 bwdx declined C513', ecase(1, 1, 513, 1, 7, 2, 3, 64)),
    ('c1 bwdx declined lens', ecase(1, 3, 16, 1, 7, 2, 3, 300, lens=2)),
    # --- epilogue options alone and combined, output / residual views ---------------------------------------------
    ('ep bias', ecase(0, 2, 24, 40, 5, 2, 2, 100, bias=1, yv='c')),
    ('ep res', ecase(0, 2, 24, 40, 5, 2, 2, 100, res=1, yv='o', rv='a')),
    ('ep gate', ecase(0, 2, 24, 40, 5, 2, 2, 100, act=G_, yv='a', rv='o')),
    ('ep lens', ecase(0, 3, 24, 40, 5, 2, 2, 100, lens=2, yv='m')),
    ('ep act', ecase(0, 2, 24, 40, 5, 2, 2, 100, act=L_, yv='h')),
    ('ep acc', ecase(0, 2, 24, 40, 5, 2, 2, 100, acc=1, yv='o')),
    ('ep all', ecase(0, 3, 24, 40, 5, 2, 2, 100, bias=1, res=1, act=L_, lens=2, acc=1, yv='o')),
    ('ep all m1 s4', ecase(1, 3, 24, 40, 8, 4, 2, 100, bias=1, res=1, act=L_, lens=2, acc=1, yv='o')),
    ('ep all m1 s2', ecase(1, 3, 24, 40, 7, 2, 3, 100, bias=1, act=G_, lens=2, acc=1, yv='a')),
    ('ep all m1 s3', ecase(1, 3, 24, 40, 7, 3, 2, 100, bias=1, res=1, act=L_, lens=2, acc=1, yv='m')),
]


def legacy_shapes(n=40, seed=77):
    """the seeded shapes of the earlier test_conv_fuzz.py, draw for draw: (kind, cin, cout, k, s, p, lin, B, opts)"""
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))
    out = []
    while len(out) < n:
        kind = 'conv' if ri(0, 1) == 0 else 'convT'
        s = [1, 2, 2, 3, 4, 4, 8][ri(0, 6)]
        k = ri(max(1, s - 1), 2 * s + 3)
        p = ri(0, k - 1) if kind == 'conv' else ri(0, min(k - 1, 5))
        cin = [1, 3, 16, 17, 24, 40, 64, 96, 130][ri(0, 8)]
        cout = [1, 5, 16, 32, 33, 70, 128, 200][ri(0, 7)]
        lin = [7, 64, 100, 256, 333, 512, 1000, 1024][ri(0, 7)]
        B = ri(1, 3)
        lout = (lin + 2 * p - k) // s + 1 if kind == 'conv' else (lin - 1) * s - 2 * p + k
        if lout < 1 or (kind == 'conv' and lin + 2 * p < k):
            continue
        opts = dict(bias=ri(0, 1), res=ri(0, 1), lens=ri(0, 1), act=ri(0, 2), acc=ri(0, 1), view=ri(0, 1))
        if opts['act'] == 2:
            opts['res'] = 1
        out.append((kind, cin, cout, k, s, p, lin, B, opts))
    return out


def _legacy_engine():
    """each legacy shape as its forward call (with its epilogue options, x in the slab view) and its backward-data call (the
    plain convolution's, into a NaN-filled dx)"""
    out = []
    for i, (kind, cin, cout, k, s, p, lin, B, o) in enumerate(legacy_shapes()):
        mode = 0 if kind == 'conv' else 1
        act = (ACT_NONE, ACT_LEAKY, ACT_LEAKY_GATE)[o['act']]
        fwd = ecase(mode, B, cin, cout, k, s, p, lin, bias=o['bias'], res=o['res'], act=act, lens=o['lens'], acc=o['acc'],
                    xv='l' if o['view'] else 'c', yv='c')
        # backward-data: the other mode, dy [B, cout, lout] -> dx [B, cin, lin]
        bwd = EC(1 - mode, B, cout, cin, k, s, p, fwd.Lout, lin, eopts(yv='c'))
        out += [('legacy %d fwd' % i, fwd), ('legacy %d bwd-data' % i, bwd)]
    return out


E_POOL = dict(s=(1, 2, 2, 3, 4, 4, 5, 8), C=(1, 2, 3, 15, 16, 17, 31, 32, 48, 64, 65, 66, 96, 130),
              O=(1, 5, 16, 31, 32, 33, 64, 65, 70, 128, 129, 200), L=(1, 3, 7, 63, 64, 65, 100, 127, 128, 129, 256, 333, 512),
              view=('c', 'a', 'o', 'h', 'm'))


def _random_engine(n, seed):
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))

    def pick(pool):
        return pool[ri(0, len(pool) - 1)]
    out = []
    while len(out) < n:
        mode, s = ri(0, 1), pick(E_POOL['s'])
        k = ri(max(1, s - 1), 2 * s + 3)
        p = ri(0, k - 1) if mode == 0 else ri(0, min(k - 1, 5))
        C, O, L, B = pick(E_POOL['C']), pick(E_POOL['O']), pick(E_POOL['L']), ri(1, 4)
        extra = ri(0, s - 1) if mode == 1 else 0
        if out_len(mode, k, s, p, L) < 1 or (mode == 0 and L + 2 * p < k):
            continue
        c = ecase(mode, B, C, O, k, s, p, L, extra=extra, bias=ri(0, 1), res=ri(0, 1), act=(N_, L_, G_)[ri(0, 2)],
                  lens=min(ri(0, 2), 2 if B >= 3 else 1), acc=ri(0, 1), xv=pick(E_POOL['view']), yv=pick(E_POOL['view']),
                  rv=pick(E_POOL['view']),
                  wp0=int(mode == 1 and ri(0, 3) == 0))
        if engine_macs(c) > MAC_MAX / 8:
            continue
        out.append(('random %d' % len(out), c))
    return out


def engine_cases(n_random=30, seed=79):
    """[(label, EC)]: the pinned classes, the 40 legacy shapes (forward + backward-data), then `n_random` seeded cases"""
    return PINNED_ENGINE + _legacy_engine() + _random_engine(n_random, seed)


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradient: dw[a,c,k] += sum_{b,t} sh[b,a,t] lg[b,c,s t + k - p]
# ---------------------------------------------------------------------------------------------------------------------
WC = collections.namedtuple('WC', 'role B A C K s p Lsh Llg o')


def wopts(shv='c', lgv='c', dw0=1, ws=None):
    """shv / lgv: view forms;  dw0: dw starts non-zero;  ws: workspace floats of a raw call as a multiple of A C K (None:
    what the wrapper binds, ag_conv1d_wgrad_ws_numel)"""
    return dict(shv=shv, lgv=lgv, dw0=dw0, ws=ws)


def wcase(role, B, cin, cout, K, s, p, lin, **kw):
    """role 'conv': the gradient of a Conv1d (cin -> cout) on an input of length lin: sh = dy, lg = x;
    'convT': of a ConvTranspose1d: sh = x, lg = dy"""
    if role == 'conv':
        return WC(role, B, cout, cin, K, s, p, (lin + 2 * p - K) // s + 1, lin, wopts(**kw))
    return WC(role, B, cin, cout, K, s, p, lin, (lin - 1) * s - 2 * p + K, wopts(**kw))


def wgrad_macs(c):
    return c.B * c.A * c.Lsh * c.C * c.K


def c1_wgrad_slabs(B, A, Lt, s, K):
    if not (s == 2 and K == 7):
        return 0, 1
    gx, gy = cdiv(Lt, 1024), cdiv(A, 8)
    gz = max(1, min(cdiv(512, gx * gy), B))
    bper = cdiv(B, gz)
    return gx * cdiv(B, bper), bper


def wgrad_ws_numel(B, A, Lsh, C, K):
    """ag_conv1d_wgrad_ws_numel"""
    if C == 1 and K <= 8:
        gx, gy = cdiv(Lsh, 256), cdiv(A, 8)
        n2 = max(1, min(cdiv(512, gx * gy), B)) * gx * A * K
        return max(n2, c1_wgrad_slabs(B, A, Lsh, 2, K)[0] * A * K) if K == 7 else n2
    CK = C * K
    AT, NT = (32, 128) if A <= 32 else ((64, 64) if (A <= 64 or CK <= 64) else (128, 128))
    TC = 32 if AT >= 128 else 64
    if Lsh < TC:
        TC = roundup(Lsh, 4)
    total = B * cdiv(Lsh, TC)
    return max(1, min(cdiv(512, cdiv(CK, NT) * cdiv(A, AT)), total)) * A * CK


def wgrad_plan(prec, c, ws_numel=None):
    """what ag_conv1d_wgrad launches; ws_numel: the bound workspace (None: what kernels.conv_wgrad binds).
    'error': the documented argument error of a workspace below one slab"""
    rb, o = prec == 'bf16', c.o
    B, A, C, K, s, p, Lsh, Llg = c.B, c.A, c.C, c.K, c.s, c.p, c.Lsh, c.Llg
    want = wgrad_ws_numel(B, A, Lsh, C, K)
    ws = want if ws_numel is None else ws_numel
    vec = vec_ok(o['shv'], A, Lsh)
    base = dict(ws_want=want, vec=vec, bf16=False, error=False, twostage=True)
    slabs, bper = c1_wgrad_slabs(B, A, Lsh, s, K)
    if C == 1 and ws > 0 and slabs > 0 and vec and ws >= slabs * A * K:
        return dict(base, kernel='conv_c1_wgrad4_kernel<2,7,8>', slabs=slabs, gz=slabs // cdiv(Lsh, 1024), TC=0, nchunk=1, tile=None)
    if C == 1 and K <= 8:
        gx, gy = cdiv(Lsh, 256), cdiv(A, 8)
        gz = max(1, min(cdiv(512, gx * gy), B))
        if ws < gx * A * K:
            return dict(base, kernel=None, error=True)
        if gz * gx * A * K > ws:
            gz = ws // (gx * A * K)
        gz = cdiv(B, cdiv(B, gz))
        return dict(base, kernel='conv_c1_wgrad_kernel<8,8>', slabs=gx * gz, gz=gz, TC=0, nchunk=1, tile=None)
    CK = C * K
    if A <= 32:
        cfg = (1, 1, 1, 4)
    elif A <= 64 or CK <= 64:
        cfg = (1, 1, 2, 2)
    else:
        cfg = (2, 2, 2, 2)
    AT, NT = 32 * cfg[0] * cfg[2], 32 * cfg[1] * cfg[3]
    n_out = A * CK
    gx, gy = cdiv(CK, NT), cdiv(A, AT)
    lgbase, lgbs, lgcs = strides(o['lgv'], C, Llg)
    refusal = None
    if rb:
        TC = 64
        span = s * (TC - 1) + K
        maxch = min((NT - 1) // K + 2, C)
        PR = ((-p) % 4 + span + 3) // 4
        lgp = roundup(2 * span, 4) + 4
        lds = 2 * ((AT * (TC * 2 + 16) + maxch * lgp + 15) & ~15)
        if Lsh % TC != 0:
            refusal = 'Lsh%64'
        elif not vec:
            refusal = 'sh unaligned'
        elif (s * TC) % 4 != 0:
            refusal = 's*TC%4'
        elif Llg % 4 != 0 or Llg < 4:
            refusal = 'Llg%4'
        elif lgcs % 4 != 0 or lgbs % 4 != 0 or lgbase % 4 != 0:
            refusal = 'lg pitch or base'
        elif AT * (TC // 4) > WB_FS * 256:
            refusal = 'WB_FS'
        elif maxch * PR > WB_FL * 256:
            refusal = 'WB_FL'
        elif lds > 160 * 1024:
            refusal = 'LDS'
        if refusal is None:
            nchunk = Lsh // TC
            gz = max(1, min(cdiv(512, gx * gy), B * nchunk))
            if ws < n_out:
                return dict(base, kernel=None, error=True)
            if gz * n_out > ws:
                gz = ws // n_out
            return dict(base, kernel='conv_wgrad_bf16_kernel<%d,%d,%d,%d>' % cfg, bf16=True, TC=TC, nchunk=nchunk, gz=gz,
                        slabs=gz, tile=(AT, NT), maxch=maxch, refusal=None)
    TC = 32 if AT >= 128 else 64
    if Lsh < TC:
        TC = roundup(Lsh, 4)
    nchunk = cdiv(Lsh, TC)
    maxch = min((NT - 1) // K + 2, C)
    lds = 2 * (TC * (AT + 1) + maxch * ((s * (TC - 1) + K) | 1)) * 4
    assert lds <= 160 * 1024, 'the tile needs more LDS than the kernel takes'
    gz = max(1, min(cdiv(512, gx * gy), B * nchunk))
    if ws < n_out:
        return dict(base, kernel=None, error=True)
    if gz * n_out > ws:
        gz = ws // n_out
    return dict(base, kernel='conv_wgrad_kernel<%d,%d,%d,%d>' % cfg, TC=TC, nchunk=nchunk, gz=gz, slabs=gz, tile=(AT, NT),
                maxch=maxch, refusal=refusal)


PINNED_WGRAD = [
    # --- tiles and roles -------------------------------------------------------------------------------------------
    ('32x128 conv', wcase('conv', 2, 24, 32, 5, 2, 2, 256)),
    ('32x128 convT', wcase('convT', 2, 32, 24, 8, 4, 2, 64, shv='a', lgv='a')),
    ('64x64 A<=64', wcase('conv', 2, 24, 64, 5, 2, 2, 256, lgv='a')),
    ('64x64 CK<=64', wcase('conv', 2, 8, 130, 7, 2, 3, 256)),                        # CK = 56
    ('64x64 convT', wcase('convT', 3, 40, 16, 8, 4, 2, 64)),
    ('128x128 conv', wcase('conv', 2, 40, 130, 3, 1, 1, 256, shv='a')),
    ('128x128 convT', wcase('convT', 2, 130, 24, 8, 4, 2, 64)),
    # --- the bf16 kernel's refusals, one at a time (each next to a shape it takes) -----------------------------------
    ('bf16 taken', wcase('conv', 2, 24, 64, 3, 1, 1, 128)),
    ('bf16 Lsh%64', wcase('conv', 2, 24, 64, 3, 1, 1, 132)),
    ('bf16 sh unaligned', wcase('conv', 2, 24, 64, 3, 1, 1, 128, shv='m')),
    ('bf16 Llg%4', wcase('conv', 2, 24, 64, 5, 2, 2, 255)),                          # Lsh = 128
    ('bf16 lg pitch', wcase('conv', 2, 24, 64, 3, 1, 1, 128, lgv='h')),
    ('bf16 lg base', wcase('conv', 2, 24, 64, 3, 1, 1, 128, lgv='m')),
    ('bf16 WB_FL', wcase('conv', 2, 24, 64, 7, 8, 3, 1024)),                         # 11 channel rows x 129 pieces > 5 x 256
    # --- time chunks, gz ----------------------------------------------------------------------------------------------
    ('Lsh<TC', wcase('conv', 2, 24, 64, 3, 1, 1, 10)),
    ('Lsh%TC', wcase('conv', 2, 24, 64, 3, 1, 1, 100)),
    ('gz = total', wcase('conv', 1, 24, 64, 3, 1, 1, 192)),                          # total = 3 chunks < cdiv(512, gx gy)
    ('gz by grid', wcase('conv', 2, 130, 200, 9, 4, 4, 2048)),                       # gx gy = 20: gz = 26 < total = 32
    ('nchunk > gz', wcase('conv', 1, 130, 129, 9, 4, 4, 6912)),                      # Lsh = 1728: 54 (bf16: 27) chunks, 26 slices
    # --- ragged edges, maxch, halos -----------------------------------------------------------------------------------
    ('A ragged both', wcase('conv', 2, 33, 129, 5, 2, 2, 200)),                      # A = 129, CK = 165
    ('maxch clipped', wcase('conv', 2, 2, 40, 9, 4, 4, 256)),                        # C = 2 < (NT - 1) / K + 2
    ('halo pad0', wcase('conv', 2, 24, 40, 7, 3, 0, 200)),
    ('halo pad K-1', wcase('conv', 2, 24, 40, 7, 3, 6, 200)),
    ('halo convT pad0', wcase('convT', 2, 24, 40, 7, 3, 0, 70)),
    ('halo convT pad', wcase('convT', 2, 24, 40, 7, 3, 5, 70)),
    # --- accumulation ----------------------------------------------------------------------------------------------
    ('dw0 zero', wcase('conv', 2, 24, 40, 5, 2, 2, 256, dw0=0)),
    # --- single-channel kernels --------------------------------------------------------------------------------------
    ('c1 wgrad4', wcase('conv', 3, 1, 16, 7, 2, 3, 2050, shv='a')),                   # Lsh = 1025: two blocks
    ('c1 wgrad4 A ragged', wcase('conv', 9, 1, 20, 7, 2, 3, 300, shv='a')),
    ('c1 generic k7 unaligned', wcase('conv', 3, 1, 16, 7, 2, 3, 2050, shv='o')),
    ('c1 generic k5', wcase('conv', 3, 1, 16, 5, 2, 2, 700)),
    ('c1 generic k8 s4', wcase('conv', 2, 1, 33, 8, 4, 2, 1000, lgv='o')),
    ('c1 k17 mfma', wcase('conv', 2, 1, 128, 17, 8, 8, 1024)),
]


def _legacy_wgrad():
    out = []
    for i, (kind, cin, cout, k, s, p, lin, B, o) in enumerate(legacy_shapes()):
        v = 'l' if o['view'] else 'c'        # (the earlier fuzz placed x in the slab and kept dy contiguous, dw zeroed)
        kw = dict(lgv=v) if kind == 'conv' else dict(shv=v)
        out.append(('legacy %d' % i, wcase(kind, B, cin, cout, k, s, p, lin, dw0=0, **kw)))
    return out


def _random_wgrad(n, seed):
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))

    def pick(pool):
        return pool[ri(0, len(pool) - 1)]
    out = []
    while len(out) < n:
        role, s = ('conv', 'convT')[ri(0, 1)], pick(E_POOL['s'])
        k = ri(max(1, s - 1), 2 * s + 3)
        p = ri(0, k - 1) if role == 'conv' else ri(0, min(k - 1, 5))
        cin, cout, L, B = pick(E_POOL['C']), pick(E_POOL['O']), pick(E_POOL['L']), ri(1, 4)
        if (role == 'conv' and L + 2 * p < k) or (role == 'convT' and (L - 1) * s - 2 * p + k < 1):
            continue
        c = wcase(role, B, cin, cout, k, s, p, L, shv=pick(E_POOL['view']), lgv=pick(E_POOL['view']), dw0=ri(0, 1))
        if wgrad_macs(c) > MAC_MAX / 8:
            continue
        out.append(('random %d' % len(out), c))
    return out


def wgrad_cases(n_random=30, seed=83):
    return PINNED_WGRAD + _legacy_wgrad() + _random_wgrad(n_random, seed)


# the shape of test_conv_wgrad_workspace_sizes: 16 slices wanted on the 128 x 128 tile, ragged in A and CK
WS_CASE = wcase('conv', 4, 40, 130, 3, 1, 1, 512, shv='a', lgv='a')


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references
# ---------------------------------------------------------------------------------------------------------------------
def _draw(pas, gen):
    if pas is EXACT:
        return lambda *s: torch.randint(-3, 4, s, generator=gen).float()
    return lambda *s: torch.randn(*s, generator=gen)


def rnd16(t):
    return t.bfloat16().float()


def engine_inputs(c, pas, seed):
    """CPU tensors of an engine case: x, w ([O,C,K] mode 0 / [C,O,K] mode 1), y0, bias, res, lens"""
    gen = torch.Generator().manual_seed(seed)
    draw, o = _draw(pas, gen), c.o
    w = draw(*((c.O, c.C, c.K) if c.mode == 0 else (c.C, c.O, c.K)))
    if pas is REAL:
        w = w / (c.C * c.K) ** 0.5
    inp = dict(x=draw(c.B, c.C, c.Lin), w=w, y0=draw(c.B, c.O, c.Lout), bias=draw(c.O) if o['bias'] else None,
               res=draw(c.B, c.O, c.Lout) if o['res'] else None, lens=None)
    if o['lens'] == 1:
        inp['lens'] = torch.randint(1, c.Lout + 1, (c.B,), generator=gen)
    elif o['lens'] == 2:
        inp['lens'] = torch.tensor([(0, c.Lout, 1, c.Lout // 2)[b % 4] for b in range(c.B)], dtype=torch.int64)
    return inp


def engine_linear(c, x, w):
    """the plain (transposed) convolution of the contract, in the dtype of its operands"""
    if c.mode == 0:
        return KM._fit(F.conv1d(x, w, None, c.s, c.p), c.Lout)
    return KM._fit(F.conv_transpose1d(x, w, None, c.s, 0)[:, :, c.p:], c.Lout)


def epilogue(c, pas, v, inp):
    """bias, residual / gate, activation, length mask, accumulate - in the dtype of v"""
    o, slope, dt = c.o, pas['slope'], v.dtype
    if inp['bias'] is not None:
        v = v + inp['bias'].to(dt).view(1, -1, 1)
    if inp['res'] is not None:
        r = inp['res'].to(dt)
        v = torch.where(r > 0, v, v * slope) if o['act'] == ACT_LEAKY_GATE else v + r
    if o['act'] == ACT_LEAKY:
        v = torch.where(v > 0, v, v * slope)
    if inp['lens'] is not None:
        v = v * (torch.arange(c.Lout).view(1, 1, -1) < inp['lens'].view(-1, 1, 1)).to(dt)
    return v + inp['y0'].to(dt) if o['acc'] else v


def engine_reference(c, pas, inp, rounded=False):
    x, w = (rnd16(inp['x']), rnd16(inp['w'])) if rounded else (inp['x'], inp['w'])
    return epilogue(c, pas, engine_linear(c, x.double(), w.double()), inp)


def wgrad_inputs(c, pas, seed):
    gen = torch.Generator().manual_seed(seed)
    draw = _draw(pas, gen)
    sh, lg, dw0 = draw(c.B, c.A, c.Lsh), draw(c.B, c.C, c.Llg), draw(c.A, c.C, c.K)
    if pas is REAL:
        sh = sh / (c.B * c.Lsh) ** 0.5          # dw of order 1, like dw0
    if not c.o['dw0']:
        dw0 = torch.zeros_like(dw0)
    return dict(sh=sh, lg=lg, dw0=dw0)


def wgrad_linear(c, sh, lg):
    """sum_{b,t} sh[b,a,t] lg[b,c,s t + k - p] (zero outside the signal): the weight gradient of a conv1d over the padded
    lg that puts out exactly Lsh steps"""
    need = c.s * (c.Lsh - 1) + c.K
    lp = F.pad(lg, (c.p, max(0, need - c.p - c.Llg)))[:, :, :need]
    w = torch.zeros(c.A, c.C, c.K, dtype=sh.dtype, requires_grad=True)
    F.conv1d(lp, w, None, c.s).backward(sh)
    return w.grad


def wgrad_reference(c, pas, inp, rounded=False):
    sh, lg = (rnd16(inp['sh']), rnd16(inp['lg'])) if rounded else (inp['sh'], inp['lg'])
    return inp['dw0'].double() + wgrad_linear(c, sh.double(), lg.double())


# ---------------------------------------------------------------------------------------------------------------------
# runners.  `Kmod`: audiogan_amd.kernels on the GPU, a model of it (tests/kernel_model.py or a mutant) on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def run_engine(Kmod, c, pas, inp, device, last_kernel=None):
    o = c.o
    d0, d1, _ = inp['w'].shape
    w = inp['w'].to(device)
    wp = torch.zeros(Kmod.wpa_numel(d0, d1, c.K) if c.mode == 0 else Kmod.wpb_numel(d0, d1, c.K, c.s), device=device)
    prep_pad = 0 if (c.mode == 1 and o['wp0']) else c.p
    Kmod.prep_conv_weight(w, wp if c.mode == 0 else None, wp if c.mode == 1 else None, c.s, prep_pad)
    x = place(inp['x'], o['xv'], device)
    res = place(inp['res'], o['rv'], device) if inp['res'] is not None else None
    fill = inp['y0'] if o['acc'] else torch.full((c.B, c.O, c.Lout), float('nan'))
    fr = Frame(c.B, c.O, c.Lout, o['yv'], device, fill)
    Kmod.conv_engine(x, wp, fr.win, c.K, c.s, c.p, c.mode, bias=inp['bias'].to(device) if inp['bias'] is not None else None,
                     res=res, lens=inp['lens'].to(device) if inp['lens'] is not None else None, act=o['act'],
                     slope=pas['slope'], accumulate=bool(o['acc']), wp_pad=prep_pad if c.mode == 1 else 0)
    name = last_kernel() if last_kernel else ''
    return dict(out=fr.window(), frame_ok=fr.untouched(), kernel=name)


def run_wgrad(Kmod, c, pas, inp, device, last_kernel=None, call=None):
    """call: replaces Kmod.conv_wgrad (the raw entry point with a workspace of the test's choosing)"""
    sh, lg = place(inp['sh'], c.o['shv'], device), place(inp['lg'], c.o['lgv'], device)
    fr = FlatFrame((c.A, c.C, c.K), device, inp['dw0'])
    (call or Kmod.conv_wgrad)(sh, lg, fr.win, c.K, c.s, c.p)
    name = last_kernel() if last_kernel else ''
    return dict(out=fr.window(), frame_ok=fr.untouched(), kernel=name)


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def floor_of(model_out, ref):
    """the fp32 CPU model's own error against the float64 reference, as a fraction of the reference's largest magnitude"""
    scale = max(float(ref.abs().max()), 1e-30)
    return float((model_out.double() - ref).abs().max()) / scale


def engine_floor(c, pas, inp, rounded=False):
    x, w = (rnd16(inp['x']), rnd16(inp['w'])) if rounded else (inp['x'], inp['w'])
    ref = engine_reference(c, pas, inp, rounded)
    return floor_of(epilogue(c, pas, engine_linear(c, x, w), inp), ref)


def wgrad_floor(c, pas, inp, rounded=False):
    sh, lg = (rnd16(inp['sh']), rnd16(inp['lg'])) if rounded else (inp['sh'], inp['lg'])
    dw = inp['dw0'].clone()
    KM.conv_wgrad(sh, lg, dw, c.K, c.s, c.p)
    return floor_of(dw, wgrad_reference(c, pas, inp, rounded))


def check(tag, pas, ref, got, floor=None, form='', output='', again=None):
    """the assertions of one pass on a runner's result; returns error / floor of the real pass (0 for the exact one)"""
    tag = (tag, pas['name'], got['kernel'])
    out = got['out']
    assert got['frame_ok'], ('wrote outside its window', tag)
    assert not bool(torch.isnan(out).any()), ('NaN in the output (an element not written, or the prior output read)', tag)
    if again is not None:
        assert torch.equal(again['out'], out) and again['kernel'] == got['kernel'], ('not reproducible', tag)
    if pas is EXACT:
        assert torch.equal(out, ref.float()), ('exact pass: output differs from the float64 reference', tag,
                                               float((out.double() - ref).abs().max()))
        return 0.0
    scale = float(ref.abs().max())
    assert scale > 0.0, ('real pass: the reference is all zero, the case checks nothing', tag)
    err = float((out.double() - ref).abs().max()) / scale
    b = bound(margin_of(form, output), floor)
    assert err <= b, ('real pass: out of bound', tag, err, floor, b)
    return err / max(floor, FLOOR_MIN)


# ---------------------------------------------------------------------------------------------------------------------
# coverage.  `seen`: [(label, case, kernel name, plan)] - on the GPU the name is what ag_last_kernel reported (and was
# asserted equal to the plan's); the host test passes the plan's own.  Every class is named here, so a change of the dispatch
# (or of the list) that stops reaching one fails instead of silently shrinking the test.
# ---------------------------------------------------------------------------------------------------------------------
def _need(what, it):
    assert any(it), ('never reached', what)


def engine_kernel_names(prec):
    """every instantiation the engine class list names, in precision mode `prec`"""
    names = set(['conv_c1_fwd_kernel<2,7,4>', 'conv_c1_bwdx_kernel<2,7,4>'])
    if prec == 'f32':
        for t, key in (('1214', (0, 0)), ('2114', (0, 0)), ('2122', (0, 0)), ('2222', (3, 1)), ('2222', (3, 0))):
            names.add('conv_engine_kernel<%d,%d,%d,%d,%d,%d>' % (TILES[t] + key))
    if prec == 'bf16':
        names |= set(['conv_engine_kernel<2,1,1,4,7,2>', 'conv_engine_kernel<2,1,2,2,2,0>'])      # the fall-backs, 8 waves and solo
        for t in ('1214', '2114', '2122', '2222'):
            names.add('conv_engine_bf16_kernel<%d,%d,%d,%d,8>' % TILES[t])
        names.add('conv_engine_bf16_kernel<2,2,2,2,16>')
    return names


def assert_engine_coverage(prec, seen):
    names = set(k for _, _, k, _ in seen)
    missing = engine_kernel_names(prec) - names
    assert not missing, (prec, 'never launched', sorted(missing))
    plans = [(c, pl) for _, c, _, pl in seen if pl['form'] != 'c1']
    # the tail launches are not what ag_last_kernel reports (the call stays named after its main launch): by the plan
    tail_names = set(pl['tail']['kernel'] for c, pl in plans if pl['tail'])
    for t in ('1122', '1141'):
        assert 'conv_engine_kernel<%d,%d,%d,%d,0,0>' % TILES[t] in tail_names, (prec, 'tail tile never launched', t)
    tiles = set(pl['tile'] for c, pl in plans)
    for t in ((32, 256), (64, 128), (128, 64), (128, 128)):
        assert t in tiles, (prec, 'main tile never launched', t)
    tails = set((pl['tile'], pl['tail']['tile']) for c, pl in plans if pl['tail'])
    for t in (((64, 128), (64, 64)), ((128, 128), (128, 32))) + ((((128, 64), (128, 32)),) if prec == 'f32' else ()):
        assert t in tails, (prec, 'main + tail pairing never launched', t)
    for n in (1, 32):
        _need((prec, 'tail of', n), (pl['tail'] and pl['tail']['n_cnt'] == n for c, pl in plans))
    _need((prec, 'tail 33: no tail launch'), (pl['n_cnt'] % 128 == 33 and not pl['tail'] and pl['tile'][0] > 32 for c, pl in plans))
    _need((prec, '8 column tiles: no tail'), (pl['n_cnt'] // 128 >= 8 and 0 < pl['n_cnt'] % 128 <= 32 and not pl['tail']
                                              and pl['tile'] == (64, 128) for c, pl in plans))
    _need((prec, 'main_cols = 0'), (pl['n_cnt'] < 128 and pl['tile'] == (64, 128) for c, pl in plans))
    fp32 = [(c, pl) for c, pl in plans if pl['form'] != 'bf16']
    keys = set(pl['key'] for c, pl in fp32)
    for k in (TAP_KEYS + (0,) if prec == 'f32' else (0, 702, 301, 200)):     # (bf16 mode: on the fall-backs to the fp32 kernel)
        assert k in keys, (prec, 'tap specialisation never launched (0: generic)', k)
    for mode in (0, 1):
        _need((prec, 'mode', mode), (c.mode == mode for c, pl in plans))
    _need((prec, 'mode 1 with Lout beyond the last scattered position'),
          (c.mode == 1 and c.Lout > out_len(1, c.K, c.s, c.p, c.Lin) for c, pl in plans))
    for s in (3, 5):
        _need((prec, 'stride', s), (c.s == s for c, pl in plans))
    _need((prec, '32 taps'), (pl['taps'] == 32 for c, pl in plans))
    _need((prec, 'K = 1'), (c.K == 1 for c, pl in plans))
    for f in (('generic', 'pipe') if prec == 'f32' else ()):
        for ch in ('one', 'several', 'last2'):
            if (f, ch) == ('pipe', 'one'):
                continue               # a single chunk is never pipelined
            _need((prec, f, ch), (pl['form'] == f and plan_class(pl, c)[1] == ch for c, pl in fp32))

    def ktot(c, pl):
        return roundup(c.C, 2) * pl['taps']
    if prec == 'f32':
        # the solo forms per tile width: the half-width and the full-width kernel are separate instantiations, each with
        # its own single-buffer chunk loop
        for tt in (64, 128):
            for f in ('solo', 'solo+dma'):
                for ch in ('one', 'several', 'last2'):
                    if (f, ch) == ('solo+dma', 'last2'):
                        continue           # DMA staging needs C % 16 == 0
                    _need((prec, f, ch, 'on tile width', tt),
                          (pl['form'] == f and pl['tile'] == (128, tt) and plan_class(pl, c)[1] == ch for c, pl in fp32))
        for cc in (16, 32):
            _need((prec, 'solo+dma with cc', cc), (pl['form'] == 'solo+dma' and pl['cc'] == cc for c, pl in fp32))
        # half-width tiles: both sides of C taps = 128.  (fp32 mode takes the full tile only with >= 512 workgroups: its limit
        # of 512 needs those over >= 65 rows and columns and a reduction of 512, 1.1e9 multiply-adds at the least, above the
        # cap of a case.  bf16 mode takes the full tile for a deep reduction whatever the grid: both sides are there, below)
        for lo, hi, solo in ((113, 128, True), (129, 144, False)):
            _need((prec, 'half-width tile, C taps in', lo, hi), (pl['form'].startswith('solo') == solo and pl['tile'] == (128, 64) and
                                                                 c.mode == 1 and lo <= ktot(c, pl) <= hi for c, pl in fp32))
    if prec == 'bf16':
        for f in ('generic', 'solo'):
            _need((prec, 'fall-back to the fp32 kernel in form', f), (pl['form'] == f for c, pl in fp32))
        # the fall-back of a deep reduction runs the fp32 kernel on the full tile: solo up to C taps = 512, 8 waves above
        for lo, hi, solo in ((497, 512, True), (513, 528, False)):
            _need((prec, 'full-width tile, C taps in', lo, hi), (pl['form'].startswith('solo') == solo and pl['tile'] == (128, 128) and
                                                                 c.mode == 1 and lo <= ktot(c, pl) <= hi for c, pl in fp32))
        _need((prec, 'full-width solo, several chunks and a last one of 2'),
              (pl['form'] == 'solo' and pl['tile'] == (128, 128) and pl['chunks'] > 2 and pl['last'] == 2 for c, pl in fp32))
        for nw, nbuf in ((8, 1), (8, 2), (16, 2)):
            _need((prec, 'NW / nbuf', nw, nbuf), (pl['form'] == 'bf16' and pl['nw'] == nw and pl['nbuf'] == nbuf for c, pl in plans))
        for C in (16, 17, 48):
            _need((prec, 'bf16 kernel at C', C), (pl['form'] == 'bf16' and c.C == C for c, pl in plans))
        _need((prec, 'fall-back: C < 16'), (pl['form'] != 'bf16' and 1 < c.C < 16 for c, pl in plans))
        _need((prec, 'fall-back: x unaligned'), (pl['form'] != 'bf16' and c.C >= 16 and not pl['xvec'] for c, pl in plans))
        _need((prec, 'fall-back: Lin % 4'), (pl['form'] != 'bf16' and c.C >= 16 and pl['xvec'] and c.Lin % 4 for c, pl in plans))
    _need((prec, 'odd C'), (c.C % 2 == 1 and c.C > 1 for c, pl in plans))
    _need((prec, 'Lin % 4 != 0'), (c.Lin % 4 != 0 for c, pl in plans))
    _need((prec, 'Lin < 4'), (1 < c.Lin < 4 for c, pl in plans))
    _need((prec, 'Lin = 1'), (c.Lin == 1 for c, pl in plans))
    _need((prec, 'x misaligned'), (c.o['xv'] in ('m', 'o') for c, pl in plans))
    _need((prec, 'x aligned pitched'), (c.o['xv'] == 'a' and pl['xvec'] for c, pl in plans))
    m1 = [(c, pl) for c, pl in plans if c.mode == 1]
    _need((prec, 'aligned scatter'), (pl['aligned'] for c, pl in m1))
    for st in (2, 4, 8):
        _need((prec, 'aligned scatter at stride', st), (pl['aligned'] and c.s == st for c, pl in m1))
    _need((prec, 'wp_pad = pad, pad % s == 0'), (not pl['aligned'] and not c.o['wp0'] and c.s > 1 and c.p % c.s == 0 for c, pl in m1))
    _need((prec, 'wp_pad = pad, an extra tap slot'), (not pl['aligned'] and not c.o['wp0'] and c.s > 1 and c.p % c.s for c, pl in m1))
    _need((prec, 'wp_pad = 0'), (c.o['wp0'] and c.p > 0 for c, pl in m1))
    # the c1 kernels and each reason they are declined
    c1f = [(c, pl) for _, c, _, pl in seen if c.mode == 0 and c.C == 1 and c.s == 2 and c.K == 7]
    _need((prec, 'c1 fwd, two blocks'), (pl['form'] == 'c1' and c.Lout > 1024 for c, pl in c1f))
    _need((prec, 'c1 fwd, 1024 outputs'), (pl['form'] == 'c1' and c.Lout == 1024 for c, pl in c1f))
    for why, f in (('res', lambda c: c.o['res'] and c.o['act'] != G_), ('accumulate', lambda c: c.o['acc']),
                   ('gate', lambda c: c.o['act'] == G_), ('y base', lambda c: c.o['yv'] == 'm'), ('y pitch', lambda c: c.o['yv'] == 'h')):
        _need((prec, 'c1 fwd declined', why), (pl['form'] != 'c1' and f(c) for c, pl in c1f))
    c1b = [(c, pl) for _, c, _, pl in seen if c.mode == 1 and c.O == 1 and c.s == 2 and c.K == 7]
    for acc in (0, 1):
        for al in (False, True):
            _need((prec, 'c1 bwdx accumulate / aligned', acc, al), (pl['form'] == 'c1' and c.o['acc'] == acc and pl['aligned'] == al for c, pl in c1b))
    _need((prec, 'c1 bwdx around 1024'), (pl['form'] == 'c1' and pl['slabs'] > 1 for c, pl in c1b))
    _need((prec, 'c1 bwdx declined: C = 513'), (pl['form'] != 'c1' and c.C == 513 for c, pl in c1b))
    _need((prec, 'c1 bwdx declined: lens'), (pl['form'] != 'c1' and c.o['lens'] for c, pl in c1b))
    # epilogue options alone and combined, views of the output and the residual
    alone = dict(bias=0, res=0, act=N_, lens=0, acc=0)
    for k, v in (('bias', 1), ('res', 1), ('lens', 2), ('act', L_), ('acc', 1)):
        want = dict(alone, **{k: v})
        _need((prec, 'epilogue option on its own', k), (all(c.o[q] == want[q] for q in want) for c, pl in plans))
    _need((prec, 'gate on its own'), (c.o['act'] == G_ and not (c.o['bias'] or c.o['lens'] or c.o['acc']) for c, pl in plans))
    for mode in (0, 1):
        _need((prec, 'all epilogue options, mode', mode),
              (c.mode == mode and c.o['bias'] and c.o['res'] and c.o['act'] == L_ and c.o['lens'] == 2 and c.o['acc'] for c, pl in plans))
    for s in (2, 3, 4):
        _need((prec, 'mode 1 epilogue with lens and accumulate at stride', s),
              (c.mode == 1 and c.s == s and c.o['lens'] == 2 and c.o['acc'] for c, pl in plans))
    for v in ('c', 'a', 'o', 'h', 'm'):
        _need((prec, 'output view', v), (c.o['yv'] == v for c, pl in plans))
    _need((prec, 'residual pitched differently from the output'), (c.o['res'] and c.o['rv'] != c.o['yv'] for c, pl in plans))


def wgrad_kernel_names(prec):
    names = set(['conv_c1_wgrad4_kernel<2,7,8>', 'conv_c1_wgrad_kernel<8,8>'])
    for cfg in ((1, 1, 1, 4), (1, 1, 2, 2), (2, 2, 2, 2)):
        names.add('conv_wgrad_kernel<%d,%d,%d,%d>' % cfg)
        if prec == 'bf16':
            names.add('conv_wgrad_bf16_kernel<%d,%d,%d,%d>' % cfg)
    return names


def assert_wgrad_coverage(prec, seen):
    names = set(k for _, _, k, _ in seen)
    missing = wgrad_kernel_names(prec) - names
    assert not missing, (prec, 'never launched', sorted(missing))
    mf = [(c, pl) for _, c, _, pl in seen if pl['tile']]
    for tile in ((32, 128), (64, 64), (128, 128)):
        for role in ('conv', 'convT'):
            _need((prec, tile, role), (pl['tile'] == tile and c.role == role for c, pl in mf))
    _need((prec, '64 x 64 by A <= 64'), (pl['tile'] == (64, 64) and 32 < c.A <= 64 and c.C * c.K > 64 for c, pl in mf))
    _need((prec, '64 x 64 by CK <= 64'), (pl['tile'] == (64, 64) and c.A > 64 for c, pl in mf))
    if prec == 'bf16':
        for why in ('Lsh%64', 'sh unaligned', 'Llg%4', 'lg pitch or base', 'WB_FL'):
            _need((prec, 'bf16 kernel refused', why), (not pl['bf16'] and pl['refusal'] == why for c, pl in mf))
        _need((prec, 'bf16 refused by the lg base alone'), (pl['refusal'] == 'lg pitch or base' and c.o['lgv'] == 'm' for c, pl in mf))
        _need((prec, 'bf16 refused by the lg pitch alone'), (pl['refusal'] == 'lg pitch or base' and c.o['lgv'] == 'h' for c, pl in mf))
    f32 = [(c, pl) for c, pl in mf if not pl['bf16']]
    _need((prec, 'Lsh < TC'), (c.Lsh < (32 if pl['tile'][0] >= 128 else 64) for c, pl in f32))
    _need((prec, 'Lsh % TC != 0'), (c.Lsh > pl['TC'] and c.Lsh % pl['TC'] for c, pl in f32))
    _need((prec, 'nchunk > gz'), (pl['nchunk'] > pl['gz'] for c, pl in mf))
    _need((prec, 'nchunk < gz'), (1 < pl['nchunk'] < pl['gz'] for c, pl in mf))
    _need((prec, 'gz = total'), (pl['gz'] == c.B * pl['nchunk'] > 1 for c, pl in mf))
    _need((prec, 'gz by the grid'), (1 < pl['gz'] < c.B * pl['nchunk'] for c, pl in mf))
    _need((prec, 'A and CK ragged'), (c.A % pl['tile'][0] and (c.C * c.K) % pl['tile'][1] and c.A > pl['tile'][0] for c, pl in mf))
    _need((prec, 'maxch clipped by C'), (c.C < (pl['tile'][1] - 1) // c.K + 2 and c.C > 1 for c, pl in mf))
    for role in ('conv', 'convT'):
        _need((prec, role, 'pad 0'), (c.role == role and c.p == 0 and c.K > 1 for c, pl in mf))
    _need((prec, 'pad = K - 1'), (c.p == c.K - 1 and c.K > 1 for c, pl in mf))
    _need((prec, 'right halo'), (c.s * (c.Lsh - 1) + c.K - 1 - c.p >= c.Llg for c, pl in mf))
    _need((prec, 'dw starts non-zero'), (c.o['dw0'] for c, pl in mf))
    _need((prec, 'dw starts zero'), (not c.o['dw0'] for c, pl in mf))
    c1 = [(c, pl) for _, c, _, pl in seen if c.C == 1]
    _need((prec, 'c1 wgrad4 over two blocks'), (pl['kernel'].startswith('conv_c1_wgrad4') and c.Lsh > 1024 for c, pl in c1))
    _need((prec, 'c1 generic, s2 k7 unaligned'), (pl['kernel'].startswith('conv_c1_wgrad_kernel') and c.K == 7 and c.s == 2 for c, pl in c1))
    _need((prec, 'c1 generic, K <= 8'), (pl['kernel'].startswith('conv_c1_wgrad_kernel') and c.K != 7 for c, pl in c1))
    _need((prec, 'C = 1, K = 17 on the MFMA path'), (pl['tile'] and c.K == 17 for c, pl in c1))


# ---------------------------------------------------------------------------------------------------------------------
# the companions of a conv layer's backward: channel_sum, leaky_bwd, conv_o1_*  (none of them reports a kernel name: the
# forms below are restated conditions only)
# ---------------------------------------------------------------------------------------------------------------------
SMALL_WS = 1 << 17         # what the wrappers bind (kernels._SMALL_WS)
SC = collections.namedtuple('SC', 'op B C L K o')


def sopts(acc=0, lens=0, add=0, bg=0, alias=0, bias=0, act=ACT_NONE, xv='a', yv='a', zv='a'):
    """xv: the first input (dy of channel_sum / leaky_bwd / o1_bwd / o1_wgrad, x of o1_fwd);  zv: the second input (y of
    leaky_bwd, x of o1_wgrad);  yv: the outputs;  bg / add / alias (leaky_bwd): bias_grad, add_into, dpre aliases dy"""
    return dict(acc=acc, lens=lens, add=add, bg=bg, alias=alias, bias=bias, act=act, xv=xv, yv=yv, zv=zv)


def scase(op, B, C, L, K=0, **kw):
    return SC(op, B, C, L, K, sopts(**kw))


def small_macs(c):
    return c.B * c.C * c.L * max(c.K, 1)


def sum_plan(c):
    nsplit = max(1, min(cdiv(c.B * c.L, 256 * 16), cdiv(2048, c.C)))
    return dict(kernel='channel_sum_kernel', nsplit=nsplit, slabs=nsplit, capped=cdiv(c.B * c.L, 4096) > cdiv(2048, c.C),
                twostage=nsplit > 1)


def leaky_plan(c):
    gx, bper = max(1, cdiv(c.L, 1024)), 1
    if c.o['bg']:
        bper = min(max(gx * c.C * c.B // 2048, 8), c.B)
    return dict(kernel='leaky_bwd_kernel', gx=gx, bper=bper, gz=cdiv(c.B, bper), slabs=gx * cdiv(c.B, bper), twostage=bool(c.o['bg']))


def o1_plan(c):
    """the vector forms need K = 3, L % 4 == 0 and 16-byte aligned rows of every [B, *, L] operand they read or write"""
    o, pad = c.o, (c.K - 1) // 2
    len_ok = c.K == 3 and pad == 1 and c.L % 4 == 0 and c.L >= 4

    def al(view, C):
        base, bs, cs = strides(view, C, c.L)
        return base % 4 == 0 and bs % 4 == 0 and (C == 1 or cs % 4 == 0)
    if c.op == 'o1_fwd':
        vec = len_ok and al(o['xv'], c.C) and al(o['yv'], 1)
        return dict(kernel='conv_o1_fwd_vec_kernel<3>' if vec else 'conv_o1_fwd_kernel', vec=vec, slabs=cdiv(c.L, 1024), twostage=False)
    if c.op == 'o1_bwd':
        vec = len_ok and al(o['xv'], 1) and al(o['yv'], c.C)
        return dict(kernel='conv_o1_bwdx_vec3_kernel' if vec else 'conv_o1_bwdx_kernel', vec=vec, slabs=cdiv(c.L, 1024), twostage=False)
    assert c.op == 'o1_wgrad'
    gx = cdiv(c.L, 1024)
    gz = max(1, min(cdiv(2048, gx * c.C), c.B))
    if gz * gx * c.C * c.K > SMALL_WS:
        gz = SMALL_WS // (gx * c.C * c.K)
    bper = cdiv(c.B, gz)
    vec = len_ok and al(o['xv'], 1) and al(o['zv'], c.C)
    return dict(kernel='conv_o1_wgrad_vec3_kernel' if vec else 'conv_o1_wgrad_kernel', vec=vec, gz=cdiv(c.B, bper), bper=bper,
                slabs=gx * cdiv(c.B, bper), by_B=cdiv(2048, gx * c.C) >= c.B, twostage=True)


def small_plan(c):
    return sum_plan(c) if c.op == 'sum' else (leaky_plan(c) if c.op == 'leaky' else o1_plan(c))


PINNED_SMALL = [
    # channel_sum: nsplit 1 and > 1, the cap cdiv(2048, C), accumulate on and off, strided dy
    ('sum nsplit1', scase('sum', 2, 5, 100, acc=1, xv='a')),
    ('sum nsplit1 acc0', scase('sum', 2, 5, 100, acc=0, xv='o')),
    ('sum nsplit4', scase('sum', 4, 16, 4000, acc=1, xv='c')),
    ('sum nsplit4 acc0', scase('sum', 4, 17, 4001, acc=0, xv='m')),
    ('sum capped', scase('sum', 3, 1025, 2731, acc=1, xv='o')),                       # wants 3 slices, cdiv(2048, C) = 2
    # leaky_bwd
    ('leaky plain', scase('leaky', 3, 5, 100, xv='a', zv='o', yv='m')),
    ('leaky lens', scase('leaky', 4, 5, 1025, lens=2, xv='o', zv='a', yv='o')),
    ('leaky add', scase('leaky', 3, 5, 1024, add=1, yv='o')),
    ('leaky alias', scase('leaky', 3, 6, 1023, alias=1, lens=2, xv='o')),
    ('leaky bg bper8', scase('leaky', 10, 4, 100, bg=1, lens=2, yv='o')),              # bper = 8 of 10 clips: 2 slabs
    ('leaky bg bper>8', scase('leaky', 40, 500, 20, bg=1, add=1)),                     # bper = 9: 5 slabs, the last one short
    ('leaky bg B<8', scase('leaky', 3, 7, 2050, bg=1, alias=1, add=1, lens=2, xv='h')),
    # conv_o1_*: the vector form and each refusal, K in {1, 5, 9}, wave-edge halos, accumulate, gz by B and by the grid
    ('o1 fwd vec', scase('o1_fwd', 2, 24, 1028, 3, bias=1, act=L_)),
    ('o1 fwd vec 4', scase('o1_fwd', 3, 5, 4, 3, bias=1)),
    ('o1 fwd vec 1020', scase('o1_fwd', 2, 17, 1020, 3)),
    ('o1 fwd vec 1024', scase('o1_fwd', 2, 16, 1024, 3, bias=1, xv='c', yv='c')),
    ('o1 fwd L%4', scase('o1_fwd', 2, 17, 1022, 3, bias=1)),
    ('o1 fwd x base', scase('o1_fwd', 2, 17, 1024, 3, xv='m')),
    ('o1 fwd x pitch', scase('o1_fwd', 2, 17, 1024, 3, xv='h')),
    ('o1 fwd y', scase('o1_fwd', 2, 17, 1024, 3, yv='m', bias=1)),
    ('o1 fwd K1', scase('o1_fwd', 2, 17, 100, 1, bias=1)),
    ('o1 fwd K5', scase('o1_fwd', 2, 17, 1028, 5, bias=1, act=L_)),
    ('o1 fwd K9', scase('o1_fwd', 2, 17, 1025, 9, xv='o', yv='o')),
    ('o1 bwd vec', scase('o1_bwd', 2, 24, 1028, 3, acc=1)),
    ('o1 bwd vec 4', scase('o1_bwd', 3, 5, 4, 3)),
    ('o1 bwd vec 1020', scase('o1_bwd', 2, 17, 1020, 3, acc=1, yv='c')),
    ('o1 bwd vec 1024', scase('o1_bwd', 2, 33, 1024, 3)),
    ('o1 bwd L%4', scase('o1_bwd', 2, 17, 1022, 3, acc=1)),
    ('o1 bwd dy base', scase('o1_bwd', 2, 17, 1024, 3, xv='m')),
    ('o1 bwd dx pitch', scase('o1_bwd', 2, 17, 1024, 3, yv='h', acc=1)),
    ('o1 bwd K1', scase('o1_bwd', 2, 17, 100, 1)),
    ('o1 bwd K5', scase('o1_bwd', 2, 17, 1028, 5, acc=1, yv='o')),
    ('o1 bwd K9', scase('o1_bwd', 2, 17, 1025, 9, xv='o')),
    ('o1 wgrad vec', scase('o1_wgrad', 5, 24, 1028, 3)),
    ('o1 wgrad vec 4', scase('o1_wgrad', 9, 5, 4, 3)),                                # 9 clips: a last group of 1 of 4 in flight
    ('o1 wgrad vec 1020', scase('o1_wgrad', 2, 17, 1020, 3, zv='c')),
    ('o1 wgrad vec 1024', scase('o1_wgrad', 3, 16, 1024, 3)),
    ('o1 wgrad gz by grid', scase('o1_wgrad', 9, 600, 64, 3)),                         # cdiv(2048, 600) = 4 slices of 3, 3, 3 clips
    ('o1 wgrad L%4', scase('o1_wgrad', 2, 17, 1022, 3)),
    ('o1 wgrad x base', scase('o1_wgrad', 2, 17, 1024, 3, zv='m')),
    ('o1 wgrad dy pitch', scase('o1_wgrad', 2, 17, 1024, 3, xv='h')),
    ('o1 wgrad K1', scase('o1_wgrad', 2, 17, 100, 1)),
    ('o1 wgrad K5', scase('o1_wgrad', 3, 17, 1028, 5, zv='o')),
    ('o1 wgrad K9', scase('o1_wgrad', 2, 17, 1025, 9, xv='o')),
]


def _random_small(n, seed):
    gen = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=gen))

    def pick(pool):
        return pool[ri(0, len(pool) - 1)]
    out = []
    views = E_POOL['view']
    while len(out) < n:
        op = pick(('sum', 'leaky', 'o1_fwd', 'o1_bwd', 'o1_wgrad'))
        B, C, L = ri(1, 9), pick((1, 3, 16, 17, 40, 130)), pick((1, 4, 7, 100, 1020, 1024, 1028, 2049, 5000))
        c = scase(op, B, C, L, pick((1, 3, 3, 5, 7, 9)) if op.startswith('o1') else 0, acc=ri(0, 1), lens=min(ri(0, 2), 2 if B >= 3 else 1), add=ri(0, 1),
                  bg=ri(0, 1), alias=ri(0, 1), bias=ri(0, 1), act=pick((N_, L_)), xv=pick(views), yv=pick(views), zv=pick(views))
        out.append(('random %d' % len(out), c))
    return out


def small_cases(n_random=30, seed=89):
    return PINNED_SMALL + _random_small(n_random, seed)


def small_inputs(c, pas, seed):
    gen = torch.Generator().manual_seed(seed)
    draw, o = _draw(pas, gen), c.o
    if c.op == 'sum':
        return dict(dy=draw(c.B, c.C, c.L), db0=draw(c.C))
    if c.op == 'leaky':
        lens = None
        if o['lens'] == 1:
            lens = torch.randint(1, c.L + 1, (c.B,), generator=gen)
        elif o['lens'] == 2:
            lens = torch.tensor([(0, c.L, 1, c.L // 2)[b % 4] for b in range(c.B)], dtype=torch.int64)
        return dict(dy=draw(c.B, c.C, c.L), y=draw(c.B, c.C, c.L), add0=draw(c.B, c.C, c.L), lens=lens)
    w = draw(1, c.C, c.K)
    if pas is REAL:
        w = w / (c.C * c.K) ** 0.5
    dy = draw(c.B, 1, c.L)
    if pas is REAL and c.op == 'o1_wgrad':
        dy = dy / (c.B * c.L) ** 0.5
    return dict(x=draw(c.B, c.C, c.L), w=w, dy=dy, bias=draw(1) if o['bias'] else None, dx0=draw(c.B, c.C, c.L))


def small_reference(c, pas, inp, rounded=False, dtype=torch.float64):
    """{output: tensor} in `dtype` (float64: the reference; float32: the floor's model)"""
    o, slope = c.o, pas['slope']
    r = rnd16 if rounded else (lambda t: t)
    if c.op == 'sum':
        s = inp['dy'].to(dtype).sum((0, 2))
        return dict(db=s + inp['db0'].to(dtype) if o['acc'] else s)
    if c.op == 'leaky':
        dy, y = inp['dy'].to(dtype), inp['y']
        g = torch.where(y > 0, dy, dy * slope)
        if inp['lens'] is not None:
            g = g * (torch.arange(c.L).view(1, 1, -1) < inp['lens'].view(-1, 1, 1)).to(dtype)
        out = dict(dpre=g)
        if o['add']:
            out['add'] = inp['add0'].to(dtype) + g
        if o['bg']:
            out['bg'] = g.sum((0, 2))
        return out
    pad = (c.K - 1) // 2
    if c.op == 'o1_fwd':
        v = F.conv1d(r(inp['x']).to(dtype), r(inp['w']).to(dtype), None, 1, pad)
        if inp['bias'] is not None:
            v = v + inp['bias'].to(dtype)
        return dict(y=torch.where(v > 0, v, v * slope) if o['act'] == ACT_LEAKY else v)
    if c.op == 'o1_bwd':
        v = F.conv_transpose1d(r(inp['dy']).to(dtype), r(inp['w']).to(dtype), None, 1, pad)
        return dict(dx=v + inp['dx0'].to(dtype) if o['acc'] else v)
    w = torch.zeros(1, c.C, c.K, dtype=dtype, requires_grad=True)
    F.conv1d(r(inp['x']).to(dtype), w, None, 1, pad).backward(r(inp['dy']).to(dtype))
    return dict(dw=w.grad)


def run_small(Kmod, c, pas, inp, device):
    """returns {output: dict(out, frame_ok, kernel)}"""
    o, nan = c.o, float('nan')
    frames = {}
    if c.op == 'sum':
        frames['db'] = FlatFrame((c.C,), device, inp['db0'] if o['acc'] else torch.full((c.C,), nan))
        Kmod.channel_sum(place(inp['dy'], o['xv'], device), frames['db'].win, accumulate=bool(o['acc']))
    elif c.op == 'leaky':
        y = place(inp['y'], o['zv'], device)
        if o['alias']:
            frames['dpre'] = Frame(c.B, c.C, c.L, o['xv'], device, inp['dy'])
            dy = frames['dpre'].win
        else:
            frames['dpre'] = Frame(c.B, c.C, c.L, o['yv'], device, torch.full((c.B, c.C, c.L), nan))
            dy = place(inp['dy'], o['xv'], device)
        if o['add']:
            frames['add'] = Frame(c.B, c.C, c.L, o['zv'], device, inp['add0'])
        if o['bg']:
            frames['bg'] = FlatFrame((c.C,), device, torch.zeros(c.C))
        Kmod.leaky_bwd(dy, y, frames['dpre'].win, lens=inp['lens'].to(device) if inp['lens'] is not None else None,
                       slope=pas['slope'], add_into=frames['add'].win if o['add'] else None,
                       bias_grad=frames['bg'].win if o['bg'] else None)
    else:
        pad, w = (c.K - 1) // 2, inp['w'].to(device)
        if c.op == 'o1_fwd':
            frames['y'] = Frame(c.B, 1, c.L, o['yv'], device, torch.full((c.B, 1, c.L), nan))
            Kmod.conv_o1_fwd(place(inp['x'], o['xv'], device), w, inp['bias'].to(device) if inp['bias'] is not None else None,
                             frames['y'].win, c.K, pad, act=o['act'], slope=pas['slope'])
        elif c.op == 'o1_bwd':
            frames['dx'] = Frame(c.B, c.C, c.L, o['yv'], device, inp['dx0'] if o['acc'] else torch.full((c.B, c.C, c.L), nan))
            Kmod.conv_o1_bwd_data(place(inp['dy'], o['xv'], device), w, frames['dx'].win, c.K, pad, accumulate=bool(o['acc']))
        else:
            frames['dw'] = FlatFrame((1, c.C, c.K), device, torch.zeros(1, c.C, c.K))
            Kmod.conv_o1_wgrad(place(inp['dy'], o['xv'], device), place(inp['x'], o['zv'], device), frames['dw'].win, c.K, pad)
    return dict((k, dict(out=f.window(), frame_ok=f.untouched(), kernel=small_plan(c)['kernel'])) for k, f in frames.items())


def assert_small_coverage(seen):
    """seen: [(label, case, plan)]"""
    def of(op):
        return [(c, pl) for _, c, pl in seen if c.op == op]
    s = of('sum')
    for acc in (0, 1):
        _need(('channel_sum nsplit 1, accumulate', acc), (pl['nsplit'] == 1 and c.o['acc'] == acc for c, pl in s))
        _need(('channel_sum nsplit > 1, accumulate', acc), (pl['nsplit'] > 1 and c.o['acc'] == acc for c, pl in s))
    _need('channel_sum capped by cdiv(2048, C)', (pl['capped'] and pl['nsplit'] > 1 for c, pl in s))
    _need('channel_sum strided dy', (c.o['xv'] != 'c' for c, pl in s))
    l = of('leaky')
    for k in ('bg', 'lens', 'add', 'alias'):
        for v in (False, True):
            _need(('leaky_bwd', k, v), (bool(c.o[k]) == v for c, pl in l))
    _need('leaky_bwd bper at its floor of 8', (c.o['bg'] and pl['bper'] == 8 and pl['gz'] > 1 for c, pl in l))
    _need('leaky_bwd bper above 8', (c.o['bg'] and pl['bper'] > 8 and pl['gz'] > 1 and c.B % pl['bper'] for c, pl in l))
    _need('leaky_bwd bper = B', (c.o['bg'] and pl['bper'] == c.B < 8 for c, pl in l))
    for L in (1023, 1024, 1025):
        _need(('leaky_bwd L', L), (c.L == L for c, pl in l))
    _need('leaky_bwd slab views', (c.o['xv'] != 'c' and c.o['yv'] != 'c' and c.o['zv'] != 'c' for c, pl in l))
    for op, views in (('o1_fwd', ('xv', 'yv')), ('o1_bwd', ('xv', 'yv')), ('o1_wgrad', ('xv', 'zv'))):
        q = of(op)
        for L in (4, 1020, 1024, 1028):
            _need((op, 'vector form at L', L), (pl['vec'] and c.L == L for c, pl in q))
        _need((op, 'scalar form: L % 4'), (not pl['vec'] and c.K == 3 and c.L % 4 for c, pl in q))
        for v in views:
            _need((op, 'scalar form: view', v), (not pl['vec'] and c.K == 3 and c.L % 4 == 0 and c.o[v] in ('m', 'h', 'o') and
                                                 all(c.o[u] in ('a', 'c') for u in views if u != v) for c, pl in q))
        for K in (1, 5, 9):
            _need((op, 'K', K), (c.K == K for c, pl in q))
        _need((op, 'C % 16'), (c.C % 16 for c, pl in q))
    for acc in (0, 1):
        for vec in (False, True):
            _need(('o1_bwd accumulate / vector', acc, vec), (c.o['acc'] == acc and pl['vec'] == vec for c, pl in of('o1_bwd')))
    _need('o1_wgrad gz limited by B', (pl['by_B'] and pl['gz'] == c.B > 1 for c, pl in of('o1_wgrad')))
    _need('o1_wgrad gz limited by the grid', (not pl['by_B'] and 1 < pl['gz'] < c.B for c, pl in of('o1_wgrad')))

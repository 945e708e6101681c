"""Shared pieces of the pointwise and reduction launch fuzz (test_pointwise_fuzz.py on the GPU, test_pointwise_fuzz_host.py
against the CPU model)  --  TEST INFRASTRUCTURE, no test functions.

The kernels of csrc/pointwise.hip, csrc/convlstm.hip and col_sum of csrc/gemm.hip, nine families:
  wn      weight_norm_fwd / weight_norm_bwd           cells   lstm_cell_*, gru_cell_*, act_bwd2d
  bce     bce_logits_* (contiguous and strided)       elem    act_fwd, act_bwd, axpby, build_zc, critic_batch
  opt     grad_norms + opt_step                       tm      time_moments_*
  tr      bct_to_tbc, tbc_to_bct, to_bf16             rd      rowdot_fwd, rowdot_bwd, col_sum
  cl      convlstm_*, layer_norm_hbfw_*
Per family (FAMILIES[name]):
  cases()               [(label, Case)]: pinned, each at the smallest shape that reaches its branch.
  plan(c, prec)         which path the call takes, restated from sizes, pitches and alignment alone (none of these kernels
                        reports a name through ag_last_kernel: the plans are restated conditions, cross-checked on the GPU
                        only where the library offers a number - ag_rowdot_bwd_ws_numel, wpa_numel / wpb_numel);
                        'kernel' is the label the error table is kept under, 'twice' asks for a second run (fixed-order
                        reductions: identical bits).
  inputs(c, pas, seed)  CPU operands of one PASS:  EXACT integers in [-3, 3] (slope 0.5; reduction length x 9 < 2^24, so
                        every fp32 order of summation is exact and bf16 holds the operands);  REAL randn.
  reference(c, pas, inp, dtype, prec)
                        {output: tensor} restated from the kernel's documented contract in `dtype` (float64: the reference;
                        tests/kernel_model.py is NOT called).
                        Special keys: '_bit' outputs that are data movement or carried state and must be bit-identical in
                        every pass; '_int' the outputs the EXACT pass checks (absent: all - present where the rest of the
                        arithmetic is transcendental); '_scale' {output: scale} where the reference cancels to zero.
  run(Kmod, c, pas, inp, device, prec)
                        every output is a window in a sentinel frame (conv_cases.Frame / FlatFrame / StridedFrame), NaN-
                        filled when the call writes, a known non-zero start when it accumulates; inputs sit in frames of
                        another filler.  -> {output: dict(out, frame_ok, kernel)}
  coverage(seen)        every class the issue names, so that none can silently drop out of the list.
sweep() walks a family with the bound rule of DESIGN.md section 2 (conv_cases.check for the exact pass; the real pass here,
because a scale can be given): floor = error of the fp32 CPU model (CpuModel below: tests/kernel_model.py run through the same
runner on the same operands) against float64 as a fraction of the reference's largest magnitude, not below 2^-24; bound = margin x floor, never above 1e-4; bf16 outputs by the GEMM fuzz's rule (2^-7,
< 2 % off the rounding)."""
import collections
import math

import torch

from tests import kernel_model as KM
from tests.conv_cases import (Frame, FlatFrame, StridedFrame, place, SENTINEL, GUARD, bound, margin_of, floor_of,  # noqa: F401
                              check, MARGIN, MARGIN_MAX, FLOOR_MIN, CEIL, EXACT, REAL, cdiv, roundup, rnd16, _draw)

ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
OPT_RMSPROP, OPT_ADAM = 0, 1
LEAKY_SLOPE = 0.01
NAN = float('nan')
EW_GRID = 4096              # ew_grid / cl_grid / ag_build_zc: blocks of 256 threads a grid-stride launch is capped at
BIG_N = EW_GRID * 256 + 1000

# (kernel label, output) -> (a margin above 16 and at most 64, the measured ratio, the reason).  None is needed: the largest
# ratio measured on the MI355X is 3.88 (profiles/pointwise_fuzz.txt).
MARGINS = {}


class Case(dict):
    __getattr__ = dict.__getitem__


def f32(v):
    """a Python number as the fp32 value the C ABI receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def nan(*shape):
    return torch.full(shape, NAN)


def out2(R, Cc, view, device, fill):
    """a [R, Cc] output window in a pitched slab (view forms of conv_cases.geom)"""
    fr = Frame(1, R, Cc, view, device, fill)
    return fr, fr.win[0]


def in2(t, view, device):
    return place(t.unsqueeze(0), view, device)[0]


def in_flat(t, device, off=0):
    """a contiguous input displaced by `off` floats from a 16-byte aligned address (its surroundings hold 99)"""
    buf = torch.full((t.numel() + GUARD + 8,), 99.0, dtype=t.dtype, device=device)
    w = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    w.copy_(t)
    return w


def pitch2(view, R, Cc):
    """(row pitch, base offset in floats from a 16-byte aligned address) of out2 / in2"""
    from tests.conv_cases import strides
    base, _, cs = strides(view, R, Cc)
    return cs, base


def results(frames, kernel, extra=None):
    r = dict((k, dict(out=f.window(), frame_ok=f.untouched(), kernel=kernel)) for k, f in frames.items())
    for k, t in (extra or {}).items():
        r[k] = dict(out=t.detach().cpu().clone(), frame_ok=True, kernel=kernel)
    return r


def _margin(form, output):
    m = MARGINS[(form, output)][0] if (form, output) in MARGINS else margin_of(form, output)
    assert MARGIN <= m <= MARGIN_MAX
    return m


def pcheck(tag, pas, ref, got, low=None, form='', output='', again=None, bit=False, scale=None):
    """the assertions of one pass on one output; returns error / floor of the real pass (0 for an exact comparison)"""
    out = got['out'].reshape(ref.shape)
    got = dict(got, out=out)
    if again is not None:
        again = dict(again, out=again['out'].reshape(ref.shape))
    tag = (tag, pas['name'], got['kernel'])
    if not out.dtype.is_floating_point:          # flag words, length tables, step counters
        assert got['frame_ok'], ('wrote outside its window', tag)
        assert torch.equal(out, ref.to(out.dtype)), ('exact pass: integer output differs from the reference', tag, out, ref)
        assert again is None or torch.equal(again['out'], out), ('not reproducible', tag)
        return 0.0
    if out.dtype == torch.bfloat16:              # the GEMM fuzz's rule
        assert got['frame_ok'], ('wrote outside its window', tag)
        want = ref.float().bfloat16()
        assert not bool((torch.isnan(out) & ~torch.isnan(want)).any()), ('NaN in the output (an element not written, or the prior output read)', tag)
        if bit or pas is EXACT:
            assert torch.equal(out.view(torch.int16), want.view(torch.int16)), ('exact pass: bf16 output is not RNE(reference)', tag)
            return 0.0
        assert not bool(torch.isinf(out).any()), ('infinity in the output', tag)
        sc = float(ref.abs().max())
        assert sc > 0.0, ('real pass: the reference is all zero, the case checks nothing', tag)
        d = (out.double() - want.double()).abs()
        assert float(d.max()) <= 2.0 ** -7 * sc, ('real pass: bf16 output', tag, float(d.max()) / sc)
        assert float((d > 0).double().mean()) < 0.02, ('real pass: bf16 output off its rounding', tag)
        return 0.0
    if bit:                                      # data movement, carried state, conversions: the very bits (signed zeros too)
        assert got['frame_ok'], ('wrote outside its window', tag)
        want = ref.float()
        assert not bool((torch.isnan(out) & ~torch.isnan(want)).any()), ('NaN in the output (an element not written, or the prior output read)', tag)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), ('exact pass: output differs in its bits from the reference', tag)
        assert again is None or torch.equal(again['out'].view(torch.int32), out.view(torch.int32)), ('not reproducible', tag)
        return 0.0
    if pas is EXACT:
        return check(tag[0], EXACT, ref, got, again=again)
    assert got['frame_ok'], ('wrote outside its window', tag)
    assert not bool(torch.isinf(out).any()), ('infinity in the output', tag)
    assert not bool(torch.isnan(out).any()), ('NaN in the output (an element not written, or the prior output read)', tag)
    if again is not None:
        assert torch.equal(again['out'], out), ('not reproducible', tag)
    sc = float(ref.abs().max()) if scale is None else float(scale)
    assert sc > 0.0, ('real pass: the reference is all zero, the case checks nothing', tag)
    floor = float((low.reshape(ref.shape).double() - ref).abs().max()) / sc
    err = float((out.double() - ref).abs().max()) / sc
    b = bound(_margin(form, output), floor)
    assert err <= b, ('real pass: out of bound', tag, err, floor, b)
    return err / max(floor, FLOOR_MIN)


def _need(what, it):
    assert any(it), ('never reached', what)


Family = collections.namedtuple('Family', 'cases plan inputs reference run coverage passes')
FAMILIES = {}
_CACHE = {}


def _both(c):
    return (EXACT, REAL)


def _real(c):
    return (REAL,)


class CpuModel(object):
    """THE FLOOR'S MODEL: audiogan_amd.kernels as tests/kernel_model.py computes it (every name not defined here is the model's own), with what
    the C ABI does to a call and the model leaves out: scalar arguments narrowed to fp32, operands rounded to bf16 in bf16
    mode, a scatter layout whose unwritten slots are left alone.  `mutate` names one mistake (see MUTANTS)."""

    def __init__(self, prec='f32', mutate=None):
        self.prec, self.mutate, self.case = prec, mutate, None

    def __getattr__(self, name):
        return getattr(KM, name)

    # -- optimiser: the ABI takes floats ------------------------------------------------------------------------------
    def grad_norms(self, params, grads, s1, s2, norms, norm_sum, flags, grad_scale=1.0, step_dev=None, finish=True):
        return KM.grad_norms(params, grads, s1, s2, norms, norm_sum, flags, f32(grad_scale), step_dev, finish)

    def opt_step(self, params, grads, s1, s2, norms, kind, lr, clip, grad_scale, a1, b2, eps, step, step_dev=None, part=None,
                 norm_sum=None, flags=None):
        f = f32
        KM.opt_step(params, grads, s1, s2, norms, kind, f(lr), f(clip), f(grad_scale), f(a1), f(b2), f(eps), step, step_dev, part,
                    norm_sum, flags)

    # -- weight norm: the kernel writes the slots of the scatter layout it owns and no other ------------------------------
    def weight_norm_fwd(self, entries):
        keep = [e['wpb'].clone() if e.get('wpb') is not None else None for e in entries]
        KM.weight_norm_fwd(entries)
        for e, old in zip(entries, keep):
            if old is None:
                continue
            rows, cols, d1, K = _wn_dims(tuple(e['v'].shape))
            s, pad = int(e.get('stride', 1)), int(e.get('pad', 0))
            idx = wn_maps(dict(rows=rows, d1=d1, K=K, s=s, pad=pad, aligned=scatter_aligned(K, s, pad)))['b'][1]
            old[idx] = e['wpb'][idx]
            e['wpb'].copy_(old)

    # -- one-output Linear: operands rounded in bf16 mode and with bf16 storage; db sums the unrounded dy ------------------
    def rowdot_fwd(self, x, w, bias, y):
        rb = self.prec == 'bf16' or x.dtype == torch.bfloat16
        KM.rowdot_fwd(rnd16(x.float()) if rb else x, rnd16(w) if rb else w, bias, y)

    def rowdot_bwd(self, dy, x, w, dx=None, dw=None, db=None, gate=False, slope=LEAKY_SLOPE, accumulate=True):
        rb = self.prec == 'bf16' or x.dtype == torch.bfloat16
        if not rb:
            return KM.rowdot_bwd(dy, x, w, dx, dw, db, gate, slope, accumulate)
        # (the gate reads x unrounded; rounding to bf16 never moves a value across zero)
        KM.rowdot_bwd(rnd16(dy), rnd16(x.float()), rnd16(w), dx, dw, db.clone() if db is not None else None, gate, slope,
                      accumulate)
        if db is not None:
            db.copy_(db + dy.sum() if accumulate else dy.sum().view(1))


def prepared(fam, ci, c, pas, prec='f32'):
    """(inputs, float64 reference, outputs of the fp32 CPU model) of a case, built once per process and shared by every sweep"""
    key = (fam, ci, pas['name'], prec)
    if key not in _CACHE:
        F = FAMILIES[fam]
        inp = F.inputs(c, pas, 1000 + ci)
        low = F.run(CpuModel(prec), c, pas, inp, 'cpu', prec) if pas is REAL else {}
        _CACHE[key] = (inp, F.reference(c, pas, inp, torch.float64, prec), dict((k, v['out']) for k, v in low.items()))
    return _CACHE[key]


def sweep(fam, Kmod, device, prec='f32', worst=None, only=None, passes=None):
    """every case of a family in its passes on `Kmod`; ends in the family's coverage assertion (unless `only` filters).
    worst: {kernel:output -> largest real-pass error / floor}"""
    F, seen = FAMILIES[fam], []
    for ci, (label, c) in enumerate(F.cases()):
        if only is not None and not only(label, c):
            continue
        pl = F.plan(c, prec)
        if hasattr(Kmod, 'case'):
            Kmod.case = c
        for pas in F.passes(c):
            if passes is not None and pas['name'] not in passes:
                continue
            inp, ref, low = prepared(fam, ci, c, pas, prec)
            got = F.run(Kmod, c, pas, inp, device, prec)
            again = F.run(Kmod, c, pas, inp, device, prec) if pl.get('twice') else None
            names = sorted((k for k in ref if not k.startswith('_')), key=lambda k: k not in ref.get('_bit', ()))     # the bit-for-bit ones first
            assert set(got) == set(names), (fam, label, sorted(got), sorted(names))
            for k in names:
                bit = k in ref.get('_bit', ())
                if pas is EXACT and '_int' in ref and k not in ref['_int'] and not bit:
                    assert got[k]['frame_ok'], ('wrote outside its window', (fam, label, k))
                    continue
                ratio = pcheck((fam, label, k), pas, ref[k], got[k], low=low.get(k), form=pl['kernel'], output=k,
                               again=again[k] if again else None, bit=bit, scale=ref.get('_scale', {}).get(k))
                if worst is not None and pas is REAL and not bit and ref[k].dtype.is_floating_point:
                    key = pl['kernel'] + ':' + k.split('.')[0]            # ('w.3': output w of table entry 3)
                    worst[key] = max(worst.get(key, 0.0), ratio)
        seen.append((label, c, pl))
    if only is None and passes is None:
        F.coverage(seen)
    return seen


def mode_invariant(Kmod, fam, label, device):
    """the outputs of one case in fp32 mode and under Kmod.precision('bf16') - for the kernels that ignore the mode"""
    F = FAMILIES[fam]
    ci, c = [(i, c) for i, (l, c) in enumerate(F.cases()) if (label(c) if callable(label) else l == label)][0]
    inp = prepared(fam, ci, c, REAL)[0]
    a = F.run(Kmod, c, REAL, inp, device, 'f32')
    with Kmod.precision('bf16'):
        b = F.run(Kmod, c, REAL, inp, device, 'f32')
    for k in a:
        assert torch.equal(a[k]['out'].view(torch.int32) if a[k]['out'].dtype == torch.float32 else a[k]['out'],
                           b[k]['out'].view(torch.int32) if b[k]['out'].dtype == torch.float32 else b[k]['out']), \
            ('the precision mode changed a kernel that ignores it', fam, label, k)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sig(t):
    return 1.0 / (1.0 + torch.exp(-t))


VIEWS = ('a', 'o', 'h', 'm')       # four pitched view forms (conv_cases.geom; 'a' and 'm' share a pitch when the row % 4 != 0)


# =====================================================================================================================
# 4. elementwise: act_fwd, act_bwd, axpby, build_zc, critic_batch
# =====================================================================================================================
def elem_cases():
    out = []
    for n in (1, 255, 257, BIG_N):
        for act in (ACT_LEAKY, ACT_TANH, ACT_NONE):
            if n == BIG_N and act != ACT_LEAKY:
                continue
            out.append(('act_fwd n%d act%d' % (n, act), Case(op='act_fwd', n=n, act=act)))
            out.append(('act_bwd n%d act%d' % (n, act), Case(op='act_bwd', n=n, act=act)))
    for n, a, b, ynan in ((1, 2.0, 3.0, 0), (255, -1.0, 0.0, 1), (257, 0.5, -2.0, 0), (BIG_N, 1.0, 1.0, 0), (257, 3.0, 0.0, 1)):
        out.append(('axpby n%d a%g b%g' % (n, a, b), Case(op='axpby', n=n, a=a, b=b, ynan=ynan)))
    for B, T, ns, es in ((2, 3, 0, 5), (2, 3, 5, 0), (3, 5, 7, 4), (1, 1, 1, 1), (3, 1031, 1000, 361)):
        out.append(('build_zc B%d T%d ns%d es%d' % (B, T, ns, es), Case(op='build_zc', B=B, T=T, ns=ns, es=es)))
    P1, P3, P8 = (2,), (2, 4, 8), (2, 4, 8, 16, 32, 64, 128, 256)

    def cb(label, **kw):
        d = dict(op='critic', nA=3, nB=2, L=256, na=1, nb=1, la=1, lb=1, prods=P3, E=0, pa=0, pb=0, oa=0, ob=0)
        d.update(kw)
        out.append(('critic ' + label, Case(**d)))
    cb('L250', L=250, prods=P1)                                  # L % 4 != 0: scalar
    cb('aligned', E=1)                                           # 16-byte path on every row
    cb('odd pitch xa', pa=1, na=0, prods=P8, E=257)              # rows of xa at an odd pitch: some rows aligned, some not
    cb('base xb', ob=1, nb=0)                                    # xb one float off
    cb('no noise', na=0, nb=0, la=0, lb=0)
    cb('nA0', nA=0, E=3)
    cb('nB0', nB=0, E=3, prods=())
    cb('L2304', L=2304, nA=1, nB=1)                              # two blocks per row, 16-byte path
    cb('L2305', L=2305, nA=1, nB=1, la=0)                        # two blocks per row, scalar
    return out


def _rounds(n):
    return cdiv(cdiv(n, 256), EW_GRID)


def elem_plan(c, prec='f32'):
    if c.op in ('act_fwd', 'act_bwd', 'axpby'):
        return dict(kernel=c.op + '_kernel', rounds=_rounds(c.n))
    if c.op == 'build_zc':
        n = c.T * c.B * (c.ns + c.es)
        return dict(kernel='build_zc_kernel', rounds=cdiv(cdiv(n, 256), min(cdiv(n, 1024), EW_GRID)))

    def side(rows, pitch_odd, off, noise):
        if rows == 0:
            return 'none'
        if c.L % 4:
            return 'scalar'
        al = [(off + r * (c.L + 1 if pitch_odd else c.L)) % 4 == 0 for r in range(rows)]
        return 'vec' if all(al) else ('scalar' if not any(al) else 'mixed')
    return dict(kernel='critic_batch_kernel', a=side(c.nA, c.pa, c.oa, c.na), b=side(c.nB, c.pb, c.ob, c.nb),
                blocks=max(1, cdiv(c.L, 2048)))


def _lens_of(gen, n, L, on):
    if not on or n == 0:
        return None
    v = torch.randint(1, L + 1, (n,), generator=gen)
    v[0] = L
    if n > 1:
        v[1] = 1
    return v


def elem_inputs(c, pas, seed):
    gen = _gen(seed)
    draw = _draw(pas, gen)
    if c.op in ('act_fwd', 'act_bwd', 'axpby'):
        x, y = draw(c.n), draw(c.n)
        for t in (x, y):
            if c.n >= 255:                 # exact zeros of both signs: the gate's convention is o > 0
                t[3], t[7] = 0.0, -0.0
        return dict(x=x, y=y)
    if c.op == 'build_zc':
        return dict(z=draw(c.B, c.T, c.ns), c=draw(c.B, c.es))
    return dict(xa=draw(c.nA, c.L), xb=draw(c.nB, c.L), na=draw(c.nA, c.L), nb=draw(c.nB, c.L),
                la=_lens_of(gen, c.nA, c.L, c.la), lb=_lens_of(gen, c.nB, c.L, c.lb),
                ca=draw(c.nA, max(c.E, 1)), cb=draw(c.nB, max(c.E, 1)))


def _ab(c, pas):
    """axpby's factors: the case's integers in the exact pass, fractions of them in the real one (b == 0 stays 0)"""
    return (c.a, c.b) if pas is EXACT else (f32(c.a * 0.3), f32(c.b * -0.7))


def elem_reference(c, pas, inp, dtype, prec='f32'):
    slope = f32(pas['slope'])
    if c.op == 'act_fwd':
        x = inp['x'].to(dtype)
        y = torch.where(x > 0, x, x * slope) if c.act == ACT_LEAKY else (torch.tanh(x) if c.act == ACT_TANH else x)
        return dict(y=y, _bit=('y',) if c.act == ACT_NONE else ())
    if c.op == 'act_bwd':
        dy, y = inp['x'].to(dtype), inp['y'].to(dtype)
        g = torch.where(y > 0, dy, dy * slope) if c.act == ACT_LEAKY else (dy * (1 - y * y) if c.act == ACT_TANH else dy)
        return dict(dx=g, _bit=('dx',) if c.act == ACT_NONE else ())
    if c.op == 'axpby':
        a, b = _ab(c, pas)
        r = a * inp['x'].to(dtype)
        return dict(y=r + b * inp['y'].to(dtype) if b != 0.0 else r)
    if c.op == 'build_zc':
        zc = torch.cat([inp['z'], inp['c'].unsqueeze(1).expand(c.B, c.T, c.es)], 2).transpose(0, 1).contiguous()
        return dict(zc=zc.to(dtype), _bit=('zc',))
    rows = [inp['xa'].to(dtype) + (inp['na'].to(dtype) if c.na else 0.0)]
    lens = [inp['la'] if inp['la'] is not None else torch.full((c.nA,), c.L, dtype=torch.int64)]
    if c.nB:
        rows.append(inp['xb'].to(dtype) + (inp['nb'].to(dtype) if c.nb else 0.0))
        lens.append(inp['lb'] if inp['lb'] is not None else torch.full((c.nB,), c.L, dtype=torch.int64))
    out = dict(x=torch.cat(rows, 0))
    bit = ['x'] if not (c.na or c.nb) else []
    if c.prods:
        ln = torch.cat(lens, 0)
        out['lens'] = torch.stack([-((-ln) // d) for d in c.prods], 0)
    if c.E:
        out['c'] = torch.cat([inp['ca'], inp['cb']] if c.nB else [inp['ca']], 0).to(dtype)
        bit.append('c')
    return dict(out, _bit=tuple(bit))


def _rows_in(t, device, pitch_odd, off):
    """[n, L] rows at pitch L (+ 1 when pitch_odd), the first `off` floats behind a 16-byte aligned address"""
    n, L = t.shape
    fr = StridedFrame((n, L), (L + 1 if pitch_odd else L, 1), off, device, t, sentinel=99.0)
    assert (GUARD + off) % 4 == off % 4
    return fr.win


def elem_run(Kmod, c, pas, inp, device, prec='f32'):
    kernel, slope = elem_plan(c)['kernel'], pas['slope']
    dev = lambda t: t.to(device) if t is not None else None  # noqa: E731
    if c.op == 'act_fwd':
        fr = FlatFrame((c.n,), device, nan(c.n))
        Kmod.act_fwd(in_flat(inp['x'], device), fr.win, c.act, slope)
        return results(dict(y=fr), kernel)
    if c.op == 'act_bwd':
        fr = FlatFrame((c.n,), device, nan(c.n))
        Kmod.act_bwd(in_flat(inp['x'], device), in_flat(inp['y'], device), fr.win, c.act, slope)
        return results(dict(dx=fr), kernel)
    if c.op == 'axpby':
        a, b = _ab(c, pas)
        fr = FlatFrame((c.n,), device, nan(c.n) if c.ynan else inp['y'])
        Kmod.axpby(in_flat(inp['x'], device), fr.win, a, b)
        return results(dict(y=fr), kernel)
    if c.op == 'build_zc':
        fr = FlatFrame((c.T, c.B, c.ns + c.es), device, nan(c.T, c.B, c.ns + c.es))
        Kmod.build_zc(in_flat(inp['z'], device), in_flat(inp['c'], device), out=fr.win)
        return results(dict(zc=fr), kernel)
    xa, xb = _rows_in(inp['xa'], device, c.pa, c.oa), _rows_in(inp['xb'], device, c.pb, c.ob) if c.nB else None
    na = _rows_in(inp['na'], device, 0, 0) if c.na else None
    nb = _rows_in(inp['nb'], device, 0, 0) if c.nb and c.nB else None
    x, lens, cc = Kmod.critic_batch(xa, na, xb, nb, dev(inp['la']), dev(inp['lb']) if c.nB else None, tuple(c.prods),
                                    dev(inp['ca']) if c.E else None, dev(inp['cb']) if c.E and c.nB else None)
    extra = dict(x=x)
    if c.prods:
        extra['lens'] = lens
    if c.E:
        extra['c'] = cc
    return results({}, kernel, extra)


def elem_coverage(seen):
    def of(op):
        return [(c, pl) for _, c, pl in seen if c.op == op]
    for op in ('act_fwd', 'act_bwd', 'axpby'):
        for n in (1, 255, 257):
            _need((op, 'n', n), (c.n == n for c, pl in of(op)))
        _need((op, 'second grid-stride round'), (pl['rounds'] == 2 for c, pl in of(op)))
    for act in (ACT_NONE, ACT_LEAKY, ACT_TANH):
        _need(('act code', act), (c.act == act for c, pl in of('act_bwd')))
    _need('axpby b == 0 over NaN', (c.b == 0.0 and c.ynan for c, pl in of('axpby')))
    z = of('build_zc')
    _need('build_zc ns = 0', (c.ns == 0 for c, pl in z))
    _need('build_zc es = 0', (c.es == 0 for c, pl in z))
    _need('build_zc coprime', (math.gcd(c.B, c.T) == math.gcd(c.B, c.ns + c.es) == math.gcd(c.T, c.ns + c.es) == 1 and c.B > 1
                               for c, pl in z))
    _need('build_zc beyond 4096 x 1024 elements', (c.T * c.B * (c.ns + c.es) > 4096 * 1024 and pl['rounds'] == 5 for c, pl in z))   # (4 below the cap)
    k = of('critic')
    _need('critic L % 4', (c.L % 4 and pl['a'] == 'scalar' for c, pl in k))
    _need('critic odd pitch on one source', (pl['a'] == 'mixed' and pl['b'] == 'vec' for c, pl in k))
    _need('critic misaligned base', (pl['b'] == 'scalar' and pl['a'] == 'vec' and c.L % 4 == 0 for c, pl in k))
    for na, nb in ((0, 1), (1, 0), (0, 0), (1, 1)):
        _need(('critic noise', na, nb), (c.na == na and c.nb == nb and c.nA and c.nB for c, pl in k))
    _need('critic nA = 0', (c.nA == 0 for c, pl in k))
    _need('critic nB = 0', (c.nB == 0 for c, pl in k))
    _need('critic lengths absent', (not c.la and not c.lb and c.prods for c, pl in k))
    for nl in (0, 1, 3, 8):
        _need(('critic stride products', nl), (len(c.prods) == nl for c, pl in k))
    for E in (1, 257):
        _need(('critic E', E), (c.E == E for c, pl in k))
    _need('critic two blocks per row, 16-byte', (pl['blocks'] == 2 and pl['a'] == 'vec' for c, pl in k))
    _need('critic two blocks per row, scalar', (pl['blocks'] == 2 and pl['a'] == 'scalar' for c, pl in k))


def _elem_passes(c):
    if c.op in ('act_fwd',) and c.act == ACT_TANH:
        return (REAL,)
    return (REAL,) if c.op == 'build_zc' else (EXACT, REAL)


FAMILIES['elem'] = Family(elem_cases, elem_plan, elem_inputs, elem_reference, elem_run, elem_coverage, _elem_passes)


# =====================================================================================================================
# 2. cells: lstm_cell_fwd / bwd, gru_cell_fwd / bwd, act_bwd2d
# =====================================================================================================================
T_STEP = 3


def _valid(mode, B):
    if mode == 'none':
        return None
    if mode == 'all':
        return torch.full((B,), T_STEP + 1, dtype=torch.int64)
    return torch.tensor([0, T_STEP + 5, T_STEP, 1, T_STEP + 1][:B] if B > 1 else [T_STEP], dtype=torch.int64)


def cells_cases():
    out = []

    def lf(H, B, valid, absent=(), big=0):
        out.append(('lstm_fwd H%d B%d %s -%s%s' % (H, B, valid, '/'.join(absent), ' big' if big else ''),
                    Case(op='lstm_fwd', H=H, B=B, valid=valid, absent=tuple(absent), big=big)))

    def lb(H, B, valid, absent=()):
        out.append(('lstm_bwd H%d B%d %s -%s' % (H, B, valid, '/'.join(absent)),
                    Case(op='lstm_bwd', H=H, B=B, valid=valid, absent=tuple(absent), big=0)))
    lf(1, 1, 'none'); lf(255, 5, 'ragged'); lf(256, 5, 'all', ['h_out']); lf(257, 5, 'ragged', ['y_out'])
    lf(600, 5, 'ragged', ['h_prev']); lf(257, 1, 'none', ['h_prev', 'y_out']); lf(257, 5, 'ragged', ['h_prev', 'h_out'])
    lf(256, 5, 'ragged', big=1)
    lb(1, 1, 'none'); lb(255, 5, 'ragged'); lb(256, 5, 'all', ['dh']); lb(257, 5, 'ragged', ['dy']); lb(600, 5, 'ragged', ['dc_next'])
    lb(257, 5, 'ragged', ['dh_pass']); lb(257, 1, 'none', ['dh', 'dc_next', 'dh_pass']); lb(256, 5, 'ragged', ['dy', 'dc_next', 'dh_pass'])
    for H in (1, 255, 256, 257, 600):
        for B in (1, 5):
            if (H, B) in ((1, 5), (600, 1), (255, 1)):
                continue
            out.append(('gru_fwd H%d B%d' % (H, B), Case(op='gru_fwd', H=H, B=B, big=int(H == 256 and B == 5))))
            out.append(('gru_bwd H%d B%d' % (H, B), Case(op='gru_bwd', H=H, B=B, big=0)))
    for rows in (1, 7):
        for cols in (1, 256, 257):
            for act in (ACT_NONE, ACT_LEAKY, ACT_TANH):
                if (rows + cols + act) % 2 and cols != 257:
                    continue
                out.append(('act_bwd2d %dx%d act%d' % (rows, cols, act), Case(op='act2d', rows=rows, cols=cols, act=act)))
    return out


CELL_OPERANDS = dict(lstm_fwd=('gates', 'c_prev', 'c_out', 'h_out', 'y_out', 'h_prev'),
                     lstm_bwd=('ga', 'c_prev', 'c_new', 'dh', 'dy', 'dc_next', 'dgates', 'dc_prev', 'dh_pass'),
                     gru_fwd=('h_prev', 'h_out'), gru_bwd=('h_prev', 'dh', 'dh_prev'))       # (gi / gh / dgi / dgh are dense by contract)


def cell_slabs(c):
    """{operand: (cols, row pitch, column offset)}: every pitched operand of a call is a column block of a slab of its own
    width, so that a row indexed with another operand's ld* lands elsewhere"""
    out = {}
    for i, name in enumerate(CELL_OPERANDS[c.op]):
        cols = 4 * c.H if name in ('gates', 'ga', 'dgates') else c.H
        out[name] = (cols, cols + 3 + 2 * i, i % 4)
    return out


def cells_plan(c, prec='f32'):
    if c.op == 'act2d':
        return dict(kernel='act_bwd2d_kernel', blocks=cdiv(c.cols, 256), pitches=[pitch2(v, c.rows, c.cols)[0] for v in ('a', 'o', 'h')])
    return dict(kernel=dict(lstm_fwd='lstm_cell_fwd_kernel', lstm_bwd='lstm_cell_bwd_kernel', gru_fwd='gru_cell_fwd_kernel',
                            gru_bwd='gru_cell_bwd_kernel')[c.op], blocks=cdiv(c.H, 256),
                pitches=[p_ for n, (cols, p_, off) in cell_slabs(c).items() if n not in c.get('absent', ())])


def cells_inputs(c, pas, seed):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    if c.op == 'act2d':
        d = _draw(pas, gen)
        y = d(c.rows, c.cols)
        if c.cols >= 256:
            y[0, 3], y[0, 7] = 0.0, -0.0
        return dict(dy=d(c.rows, c.cols), y=y)
    B, H = c.B, c.H
    if c.op == 'lstm_fwd':
        g = r(B, 4 * H)
        if c.big:                      # pre-activations of +-30 and +-100 in every gate block
            for k, v in enumerate((30.0, -30.0, 100.0, -100.0)):
                g[:, k::7] = v
                g[:, 4 * H - 1 - k] = v
        return dict(gates=g, c_prev=r(B, H), h_prev=r(B, H))
    if c.op == 'lstm_bwd':
        pre = r(B, 4 * H)
        ga = torch.cat([sig(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])], 1)
        return dict(ga=ga, c_prev=r(B, H), c_new=r(B, H), dh=r(B, H), dy=r(B, H), dc_next=r(B, H))
    if c.op == 'gru_fwd':
        gi, gh = r(B, 3 * H), r(B, 3 * H)
        if c.big:
            for k, v in enumerate((30.0, -30.0, 100.0, -100.0)):
                gi[:, k::9] = v
        return dict(gi=gi, gh=gh, h_prev=r(B, H))
    pre = r(B, 3 * H)
    return dict(ga=torch.cat([sig(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:])], 1), gh=r(B, 3 * H), h_prev=r(B, H), dh=r(B, H))


def _padrows(c):
    v = _valid(c.valid, c.B)
    return (T_STEP >= v) if v is not None else torch.zeros(c.B, dtype=torch.bool)


def cells_reference(c, pas, inp, dtype, prec='f32'):
    if c.op == 'act2d':
        slope = f32(pas['slope'])
        dy, y = inp['dy'].to(dtype), inp['y'].to(dtype)
        g = torch.where(y > 0, dy, dy * slope) if c.act == ACT_LEAKY else (dy * (1 - y * y) if c.act == ACT_TANH else dy)
        return dict(dx=g, _bit=('dx',) if c.act == ACT_NONE else ())
    H, B = c.H, c.B
    t = dict((k, v.to(dtype)) for k, v in inp.items())
    z = torch.zeros(B, H, dtype=dtype)
    if c.op in ('lstm_fwd', 'lstm_bwd'):
        pad = _padrows(c)
        keep, pm = (~pad).view(B, 1), pad.view(B, 1)
    if c.op == 'lstm_fwd':
        g = t['gates']
        ia, fa, ga, oa = sig(g[:, :H]), sig(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
        cn = fa * t['c_prev'] + ia * ga
        hn = oa * torch.tanh(cn)
        hp = t['h_prev'] if 'h_prev' not in c.absent else z
        out = dict(gates=torch.where(keep, torch.cat([ia, fa, ga, oa], 1), g), c_out=torch.where(keep, cn, t['c_prev']))
        if 'h_out' not in c.absent:
            out['h_out'] = torch.where(keep, hn, hp)
        if 'y_out' not in c.absent:
            out['y_out'] = torch.where(keep, hn, z)
        bit = []
        if bool(pad.any()):                 # padded rows: gates untouched, c and h carried, y zero - bit for bit
            for k in list(out):
                out[k + '_pad'] = out[k][pad]
                bit.append(k + '_pad')
        return dict(out, _bit=tuple(bit))
    if c.op == 'lstm_bwd':
        ga = t['ga']
        ig, fg, gg, og = ga[:, :H], ga[:, H:2 * H], ga[:, 2 * H:3 * H], ga[:, 3 * H:]
        dhf = t['dh'] if 'dh' not in c.absent else z
        dcn = t['dc_next'] if 'dc_next' not in c.absent else z
        dhv = dhf + (t['dy'] if 'dy' not in c.absent else z)
        tc = torch.tanh(t['c_new'])
        dc = dcn + dhv * og * (1 - tc * tc)
        dg = torch.cat([dc * gg * ig * (1 - ig), dc * t['c_prev'] * fg * (1 - fg), dc * ig * (1 - gg * gg), dhv * tc * og * (1 - og)], 1)
        out = dict(dgates=torch.where(keep, dg, torch.zeros_like(dg)), dc_prev=torch.where(keep, dc * fg, dcn))
        if 'dh_pass' not in c.absent:
            out['dh_pass'] = torch.where(keep, z, dhf)
        bit = ['dh_pass'] if 'dh_pass' in out else []      # zero at a live step, dh carried at a padded one: never arithmetic
        if bool(pad.any()):
            for k in list(out):
                out[k + '_pad'] = out[k][pad]
                bit.append(k + '_pad')
        return dict(out, _bit=tuple(bit))
    if c.op == 'gru_fwd':
        gi, gh = t['gi'], t['gh']
        r = sig(gi[:, :H] + gh[:, :H])
        zz = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return dict(gi=torch.cat([r, zz, n], 1), h_out=(1 - zz) * n + zz * t['h_prev'])
    ga = t['ga']
    r, zz, n = ga[:, :H], ga[:, H:2 * H], ga[:, 2 * H:]
    dn = t['dh'] * (1 - zz) * (1 - n * n)
    dz = t['dh'] * (t['h_prev'] - n) * zz * (1 - zz)
    dr = dn * t['gh'][:, 2 * H:] * r * (1 - r)
    return dict(dgi=torch.cat([dr, dz, dn], 1), dgh=torch.cat([dr, dz, dn * r], 1), dh_prev=t['dh'] * zz)


def cells_run(Kmod, c, pas, inp, device, prec='f32'):
    kernel = cells_plan(c)['kernel']
    if c.op == 'act2d':
        fr, dx = out2(c.rows, c.cols, 'h', device, nan(c.rows, c.cols))
        Kmod.act_bwd2d(in2(inp['dy'], 'a', device), in2(inp['y'], 'o', device), dx, c.act, pas['slope'])
        return results(dict(dx=fr), kernel)
    B, H = c.B, c.H
    slabs = cell_slabs(c)
    frames = {}

    def opt(name, view=None):
        if name in c.get('absent', ()):
            return None
        cols, pitch, off = slabs[name]
        return StridedFrame((B, cols), (pitch, 1), off, device, inp[name], sentinel=99.0).win

    def outw(name, view=None, cols=H, fill=None):
        if name in c.get('absent', ()):
            return None
        cols, pitch, off = slabs[name]
        frames[name] = StridedFrame((B, cols), (pitch, 1), off, device, nan(B, cols) if fill is None else fill)
        return frames[name].win
    if c.op in ('lstm_fwd', 'lstm_bwd'):
        v = _valid(c.valid, B)
        v = v.to(device) if v is not None else None
        pad = _padrows(c)
    if c.op == 'lstm_fwd':
        g = outw('gates', 'a', 4 * H, inp['gates'])
        Kmod.lstm_cell_fwd(g, opt('c_prev'), outw('c_out', 'h'), h_out=outw('h_out', 'm'), y_out=outw('y_out', 'o'),
                           h_prev=opt('h_prev', 'a'), valid=v, t=T_STEP)
    elif c.op == 'lstm_bwd':
        Kmod.lstm_cell_bwd(opt('ga'), opt('c_prev'), opt('c_new'),
                           opt('dh', 'm'), opt('dy', 'o'), opt('dc_next', 'a'), outw('dgates', 'h', 4 * H), outw('dc_prev', 'm'),
                           dh_pass=outw('dh_pass', 'o'), valid=v, t=T_STEP)
    elif c.op == 'gru_fwd':
        frames['gi'] = FlatFrame((B, 3 * H), device, inp['gi'])
        Kmod.gru_cell_fwd(frames['gi'].win, in_flat(inp['gh'], device), opt('h_prev'), outw('h_out', 'h'))
    else:
        frames['dgi'], frames['dgh'] = FlatFrame((B, 3 * H), device, nan(B, 3 * H)), FlatFrame((B, 3 * H), device, nan(B, 3 * H))
        Kmod.gru_cell_bwd(in_flat(inp['ga'], device), in_flat(inp['gh'], device), opt('h_prev'),
                          opt('dh'), frames['dgi'].win, frames['dgh'].win, outw('dh_prev', 'o'))
    res = results(frames, kernel)
    if c.op in ('lstm_fwd', 'lstm_bwd') and bool(pad.any()):
        for k in list(res):
            res[k + '_pad'] = dict(res[k], out=res[k]['out'].reshape(B, -1)[pad])
    return res


def cells_coverage(seen):
    def of(op):
        return [(c, pl) for _, c, pl in seen if c.op == op]
    for op in ('lstm_fwd', 'lstm_bwd', 'gru_fwd', 'gru_bwd'):
        for H in (1, 255, 256, 257, 600):
            _need((op, 'H', H), (c.H == H for c, pl in of(op)))
        for B in (1, 5):
            _need((op, 'B', B), (c.B == B for c, pl in of(op)))
        _need((op, 'three column blocks'), (pl['blocks'] == 3 for c, pl in of(op)))
    for op, names in (('lstm_fwd', ('h_out', 'y_out', 'h_prev')), ('lstm_bwd', ('dh', 'dy', 'dc_next', 'dh_pass'))):
        for v in ('none', 'all', 'ragged'):
            _need((op, 'valid', v), (c.valid == v for c, pl in of(op)))
        for n in names:
            _need((op, 'absent alone', n), (c.absent == (n,) for c, pl in of(op)))
        _need((op, 'all absent that may be'), (len(c.absent) == len(names) - 1 for c, pl in of(op)))
        _need((op, 'padded rows and live rows in one call'), (c.valid == 'ragged' and c.B == 5 for c, pl in of(op)))
    _need('lstm_fwd h carried as 0 without h_prev', (c.valid == 'ragged' and 'h_prev' in c.absent and 'h_out' not in c.absent
                                                     for c, pl in of('lstm_fwd')))
    _need('lstm_fwd +-30 / +-100', (c.big for c, pl in of('lstm_fwd')))
    _need('gru_fwd +-30 / +-100', (c.big for c, pl in of('gru_fwd')))
    a = of('act2d')
    for cols in (1, 256, 257):
        for rows in (1, 7):
            _need(('act_bwd2d', rows, cols), (c.rows == rows and c.cols == cols for c, pl in a))
    for act in (ACT_NONE, ACT_LEAKY, ACT_TANH):
        _need(('act_bwd2d act', act), (c.act == act for c, pl in a))
    for label, c, pl in seen:
        assert len(set(pl['pitches'])) == len(pl['pitches']) and min(pl['pitches']) > (c.cols if c.op == 'act2d' else c.H), \
            ('every pitched operand of a call has a pitch of its own, wider than its row', label, pl['pitches'])


FAMILIES['cells'] = Family(cells_cases, cells_plan, cells_inputs, cells_reference, cells_run, cells_coverage,
                           lambda c: (EXACT, REAL) if c.op == 'act2d' else (REAL,))


# =====================================================================================================================
# 3. losses: bce_logits_fwd / bwd (contiguous rows) and the one-launch strided forms
# =====================================================================================================================
LOSS_START = 2.5
BCE_SCALE = 0.75


def bce_cases():
    out = []
    Ts, Bs = (1, 63, 64, 65, 257, 1030), (1, 3, 4, 5, 16, 17, 33)
    k = 0
    for i, T in enumerate(Ts):
        for j, B in enumerate(Bs):
            if (i + j) % 3 and not (T == 1030 and B in (17, 33)) and not (T == 65 and B == 16):
                continue
            k += 1
            nf = 'over' if (T, B) == (64, 16) else ('none', 'full', 'ragged')[k % 3]
            tg = (0.0, 0.5, 0.9)[k % 3 if k % 2 else (k + 1) % 3]
            big = int(T == 257 and B == 4) or int(T == 65 and B == 16)
            for form in ('contig', 'strided'):
                d = Case(op='bce_' + form, T=T, B=B, nf=nf, tg=tg, gs=k % 2, big=big, xv=VIEWS[k % 4], dv=VIEWS[(k + 1) % 4],
                         rows=0, per=1, sx='bt', sd='bt')
                if form == 'strided':
                    d.update(rows=int(k % 2 == 0), per=int(k % 3 != 0), sx=('tb', 'bt', 'nn')[k % 3], sd=('bt', 'tb', 'nn')[k % 3])
                out.append(('%s T%d B%d nf-%s tg%g%s' % (d.op, T, B, nf, tg, ' big' if big else ''), d))
    return out


def bce_plan(c, prec='f32'):
    if c.op == 'bce_contig':
        return dict(kernel='bce_fwd_kernel+finish / bce_bwd_kernel', twice=True, blocks=cdiv(c.B, 4), tblocks=cdiv(c.T, 256))
    return dict(kernel='bce_fwd_one_kernel / bce_bwd_strided_kernel', twice=True, rounds=cdiv(c.B, 16), tfast=c.sd == 'bt')


def bce_inputs(c, pas, seed):
    gen = _gen(seed)
    x = torch.randn(c.B, c.T, generator=gen) * 2
    if c.big:
        for k, v in enumerate((80.0, -80.0, 100.0, -100.0)):
            x[:, k::11] = v
    nf = None
    if c.nf == 'full':
        nf = torch.full((c.B,), c.T, dtype=torch.int64)
    elif c.nf in ('ragged', 'over'):
        nf = torch.randint(1, c.T + 1, (c.B,), generator=gen)
        nf[0] = c.T
        nf[-1] = 1
        if c.nf == 'over':      # a stored count above T (the reference's audiogan.py:126 / :143: every column weighs 1 and the
            nf[1], nf[2] = c.T + 3, 2 * c.T      # row's sum is divided by the stored count) - the kernels do the same
    return dict(x=x, nf=nf, rows=torch.tensor([(0.0, 0.9, 0.5)[b % 3] for b in range(c.B)]), gscale=torch.tensor([0.6]))


def bce_reference(c, pas, inp, dtype, prec='f32'):
    x = inp['x'].to(dtype)
    n = (inp['nf'] if inp['nf'] is not None else torch.full((c.B,), c.T, dtype=torch.int64))
    mask = (torch.arange(c.T).view(1, -1) < n.view(-1, 1))
    tg = inp['rows'].to(dtype).view(-1, 1) if c.rows else torch.full((c.B, 1), f32(c.tg), dtype=dtype)
    m = (-x).clamp(min=0)
    el = x - x * tg + m + torch.log(torch.exp(-m) + torch.exp(-x - m))
    per = (el * mask).sum(1)
    scale = f32(BCE_SCALE)
    val = scale * (per / n.to(dtype)).sum()
    gs = inp['gscale'].to(dtype)[0] if c.gs else 1.0
    dx = gs * scale / n.to(dtype).view(-1, 1) * (sig(x) - tg) * mask
    out = dict(loss=(val + LOSS_START if c.op == 'bce_contig' else val).view(1), dx=dx)
    if c.per:
        out['per'] = per
    return out


def _strided2(kind, B, T):
    """(strides, span offset) of a [B, T] view: 'bt' rows at a pitch, 'tb' the transpose of [T, B + 1] rows, 'nn' no unit stride"""
    return dict(bt=((T + 3, 1), 1), tb=((1, B + 1), 2), nn=((2 * T + 3, 2), 1))[kind]


def bce_run(Kmod, c, pas, inp, device, prec='f32'):
    kernel = bce_plan(c)['kernel']
    nf = inp['nf'].to(device) if inp['nf'] is not None else None
    gs = inp['gscale'].to(device) if c.gs else None
    frames = {}
    if c.op == 'bce_contig':
        frames['loss'] = FlatFrame((1,), device, torch.tensor([LOSS_START]))
        frames['per'] = FlatFrame((c.B,), device, nan(c.B))
        x = in2(inp['x'], c.xv, device)
        frames['dx'], dx = out2(c.B, c.T, c.dv, device, nan(c.B, c.T))
        Kmod.bce_logits_fwd(x, c.tg, nf, frames['per'].win, frames['loss'].win, BCE_SCALE)
        Kmod.bce_logits_bwd(x, c.tg, nf, gs, BCE_SCALE, dx)
        return results(frames, kernel)
    st, off = _strided2(c.sx, c.B, c.T)
    x = StridedFrame((c.B, c.T), st, off, device, inp['x'], sentinel=99.0).win
    st, off = _strided2(c.sd, c.B, c.T)
    frames['dx'] = StridedFrame((c.B, c.T), st, off, device, nan(c.B, c.T))
    frames['loss'] = FlatFrame((1,), device, nan(1))
    if c.per:
        frames['per'] = FlatFrame((c.B,), device, nan(c.B))
    rows = inp['rows'].to(device) if c.rows else None
    Kmod.bce_logits_fwd_strided(x, c.tg, nf, frames['per'].win if c.per else None, frames['loss'].win, BCE_SCALE, target_rows=rows)
    Kmod.bce_logits_bwd_strided(x, c.tg, nf, gs, BCE_SCALE, frames['dx'].win, target_rows=rows)
    return results(frames, kernel)


def bce_coverage(seen):
    for op in ('bce_contig', 'bce_strided'):
        q = [(c, pl) for _, c, pl in seen if c.op == op]
        for T in (1, 63, 64, 65, 257, 1030):
            _need((op, 'T', T), (c.T == T for c, pl in q))
        for B in (1, 3, 4, 5, 16, 17, 33):
            _need((op, 'B', B), (c.B == B for c, pl in q))
        for nf in ('none', 'full', 'ragged', 'over'):
            _need((op, 'nframes', nf), (c.nf == nf for c, pl in q))
        for tg in (0.0, 0.5, 0.9):
            _need((op, 'target', tg), (c.tg == tg for c, pl in q))
        for gs in (0, 1):
            _need((op, 'gscale', gs), (c.gs == gs for c, pl in q))
        _need((op, '+-80 / +-100'), (c.big for c, pl in q))
    s = [(c, pl) for _, c, pl in seen if c.op == 'bce_strided']
    for k in ('tb', 'bt', 'nn'):
        _need(('strided x', k), (c.sx == k for c, pl in s))
        _need(('strided dx', k), (c.sd == k for c, pl in s))
    _need('strided: rows beyond the 16 waves', (pl['rounds'] == 3 for c, pl in s))
    _need('strided: per-row targets', (c.rows for c, pl in s))
    _need('strided: per_sample absent', (not c.per for c, pl in s))
    t = [(c, pl) for _, c, pl in seen if c.op == 'bce_contig']
    _need('contig: pitched ldx / lddx', (pitch2(c.xv, c.B, c.T)[0] != pitch2(c.dv, c.B, c.T)[0] > c.T for c, pl in t))
    _need('contig: several time blocks', (pl['tblocks'] == 5 for c, pl in t))


FAMILIES['bce'] = Family(bce_cases, bce_plan, bce_inputs, bce_reference, bce_run, bce_coverage, _real)


# =====================================================================================================================
# 5. optimiser: grad_norms + opt_step on slices of flat buffers
# =====================================================================================================================
OPT_CHUNKS = 256
OPT_STRIPE = OPT_CHUNKS * 256        # elements one pass of the (256, n) grid covers on the scalar path
OPT_SIZES = (1, 3, 4, 255, 256, 257, 1024, 65536, 65537, 131076)
LR, A1, B2, EPS = 1e-3, 0.9, 0.999, 1e-6
STEP0 = 41                           # the device counter's start
FLAG_GARBAGE = 0x5A5A


class SliceFrame(object):
    """tensors of `sizes` as slices of one flat buffer, sentinel floats between them; slice i starts `disps[i]` floats
    behind a 16-byte aligned address"""

    def __init__(self, sizes, disps, device, fills):
        self.at, cur = [], 0
        for n, d in zip(sizes, disps):
            start = roundup(cur, 4) + 8 + d
            self.at.append((GUARD + start, n))
            cur = start + n
        self.buf = torch.full((cur + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
        self.wins = [self.buf[a:a + n] for a, n in self.at]
        self.fill(fills)
        self.before = self.buf.cpu().clone()

    def fill(self, fills):
        for w, f in zip(self.wins, fills):
            w.copy_(f)

    def untouched(self):
        after, before = self.buf.cpu().clone(), self.before.clone()
        for t in (after, before):
            for a, n in self.at:
                t[a:a + n] = 0
        return torch.equal(after.view(torch.int32), before.view(torch.int32))

    def window(self):
        return torch.cat([w.cpu() for w in self.wins])


def opt_cases():
    out = []
    al = [(0, 0, 0, 0)] * len(OPT_SIZES)
    one = [1024, 1024, 1024, 1024, 1024, 256]
    disp = [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (0, 0, 0, 0), (0, 0, 0, 0)]

    def oc(label, **kw):
        d = dict(op='opt', kind=OPT_ADAM, sizes=list(OPT_SIZES), disps=al, clip=0.0, gs=1.0, stepdev=0, flag=None, norms_only=0,
                 steps=3, exact=0)
        d.update(kw)
        out.append((label, Case(**d)))
    oc('rmsprop all sizes', kind=OPT_RMSPROP)
    oc('adam all sizes clip gs dev', clip=10.0, gs=0.125, stepdev=1)       # norms 0.1 .. 45: some tensors clipped, some not
    oc('adam displaced clip below', sizes=one, disps=disp, clip=1.0)
    oc('rmsprop displaced clip above', kind=OPT_RMSPROP, sizes=one, disps=disp, clip=1e6, stepdev=1)
    fs = [257, 1024, 4]
    fd = [(0, 0, 0, 0)] * 3
    oc('flag nan scalar-path last', sizes=fs, disps=fd, flag=(0, 256, NAN), norms_only=1, steps=1)
    oc('flag nan vector-path', sizes=fs, disps=fd, flag=(1, 517, NAN), norms_only=1, steps=1)
    oc('flag inf', sizes=fs, disps=fd, flag=(2, 1, float('inf')), norms_only=1, steps=1)
    oc('flag just above 1e5', sizes=fs, disps=fd, flag=(1, 100, 8.0001e5), gs=0.125, clip=10.0)
    oc('flag just below 1e5', sizes=fs, disps=fd, flag=(0, 100, 7.9999e5), gs=0.125, kind=OPT_RMSPROP)
    oc('norms exact', sizes=[1, 4, 256, 1024, 65536], disps=[(0, 0, 0, 0)] * 4 + [(0, 1, 0, 0)], norms_only=1, steps=1, exact=1)
    return out


def opt_plan(c, prec='f32'):
    adam = c.kind == OPT_ADAM
    npath = ['vec' if d[1] == 0 and n % 4 == 0 else 'scalar' for n, d in zip(c.sizes, c.disps)]
    spath = ['vec' if (d[0] | d[1] | d[2] | (d[3] if adam else 0)) == 0 and n % 4 == 0 else 'scalar' for n, d in zip(c.sizes, c.disps)]
    return dict(kernel='grad_norms_kernel' if c.norms_only else 'grad_norms_kernel / opt_step_kernel', twice=True, npath=npath,
                spath=spath)


EXACT_MAG = {1: 3.0, 4: 1.0, 256: 2.0, 1024: 3.0, 65536: 1.0}        # n k^2 is a perfect square


def opt_inputs(c, pas, seed):
    gen = _gen(seed)
    r = lambda n: torch.randn(n, generator=gen)  # noqa: E731
    if c.exact:
        g = [[(torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1) * EXACT_MAG[n] for n in c.sizes]]
    else:
        g = [[r(n) for n in c.sizes] for _ in range(c.steps)]
    if c.flag is not None:
        i, e, v = c.flag
        g[-1][i][e] = v
    return dict(p=[r(n) for n in c.sizes], g=g)


def opt_reference(c, pas, inp, dtype, prec='f32'):
    gs, adam, nt = f32(c.gs), c.kind == OPT_ADAM, len(c.sizes)
    p = [t.to(dtype).clone() for t in inp['p']]
    s1, s2 = [torch.zeros(n, dtype=dtype) for n in c.sizes], [torch.zeros(n, dtype=dtype) for n in c.sizes]
    lr, a1, b2, eps, clip = f32(LR), f32(A1), f32(B2), f32(EPS), f32(c.clip)
    for k in range(c.steps):
        gk = [t.to(dtype) * gs for t in inp['g'][k]]
        norms = torch.stack([(g * g).sum().sqrt() for g in gk])
        g32 = [t * gs for t in inp['g'][k]]                     # the flag tests look at the fp32 product
        flags = (1 if any(bool((g != g).any()) for g in g32) else 0) | (2 if any(bool((g.abs() > 1e5).any()) for g in g32) else 0)
        if c.norms_only:
            break
        step = STEP0 + k + 1 if c.stepdev else k + 1
        for i in range(nt):
            g = gk[i]
            if clip > 0 and float(norms[i]) > clip:
                g = g / (norms[i] / clip)
            if adam:
                s1[i] = a1 * s1[i] + (1 - a1) * g
                s2[i] = b2 * s2[i] + (1 - b2) * g * g
                p[i] = p[i] - (lr / (1 - a1 ** step)) * (s1[i] / (s2[i].sqrt() / math.sqrt(1 - b2 ** step) + eps))
            else:
                s1[i] = a1 * s1[i] + (1 - a1) * g * g
                p[i] = p[i] - lr * (g / (s1[i].sqrt() + eps))
    bad = ~torch.isfinite(norms)
    out = dict(norms=torch.where(bad, torch.zeros_like(norms), norms), nonfinite=bad.to(torch.int32),
               flags=torch.tensor([flags], dtype=torch.int32))
    if not bool(bad.any()):
        out['norm_sum'] = norms.sum().view(1)
    if c.stepdev:
        out['step'] = torch.tensor([STEP0 + c.steps], dtype=torch.int32)
    if not c.norms_only:
        out.update(p=torch.cat(p), s1=torch.cat(s1))
        if adam:
            out['s2'] = torch.cat(s2)
    return out


def _opt_once(Kmod, c, inp, device, fused):
    adam, nt = c.kind == OPT_ADAM, len(c.sizes)
    z = [torch.zeros(n) for n in c.sizes]
    P = SliceFrame(c.sizes, [d[0] for d in c.disps], device, inp['p'])
    G = SliceFrame(c.sizes, [d[1] for d in c.disps], device, inp['g'][0])
    S1 = SliceFrame(c.sizes, [d[2] for d in c.disps], device, z)
    S2 = SliceFrame(c.sizes, [d[3] for d in c.disps], device, z)
    norms, nsum = FlatFrame((nt,), device, nan(nt)), FlatFrame((1,), device, nan(1))
    flags = FlatFrame((1,), device, torch.tensor([FLAG_GARBAGE], dtype=torch.int32), dtype=torch.int32)
    step = FlatFrame((1,), device, torch.tensor([STEP0], dtype=torch.int32), dtype=torch.int32)
    sd = step.win if c.stepdev else None
    for k in range(c.steps):
        G.fill(inp['g'][k])
        ws = Kmod.grad_norms(P.wins, G.wins, S1.wins, S2.wins if adam else None, norms.win, nsum.win, flags.win, grad_scale=c.gs,
                             step_dev=sd, finish=not fused)
        if c.norms_only:
            break
        Kmod.opt_step(P.wins, G.wins, S1.wins, S2.wins if adam else None, norms.win, c.kind, LR, c.clip, c.gs, A1, B2, EPS, k + 1,
                      step_dev=sd, part=ws if fused else None, norm_sum=nsum.win, flags=flags.win)
    kernel = opt_plan(c)['kernel']
    assert G.untouched() and torch.equal(G.window().view(torch.int32), torch.cat(inp['g'][k]).view(torch.int32)), 'the gradients were written'
    frames = dict(flags=flags)
    if c.stepdev:
        frames['step'] = step
    else:
        assert step.untouched() and int(step.window()) == STEP0
    if not c.norms_only:
        frames.update(p=P, s1=S1)
        if adam:
            frames['s2'] = S2
    res = results(frames, kernel)
    nv = norms.window()
    bad = ~torch.isfinite(nv)
    ok = norms.untouched() and nsum.untouched()
    res['norms'] = dict(out=torch.where(bad, torch.zeros_like(nv), nv), frame_ok=ok, kernel=kernel)
    res['nonfinite'] = dict(out=bad.to(torch.int32), frame_ok=True, kernel=kernel)
    if not bool(bad.any()):
        res['norm_sum'] = dict(out=nsum.window(), frame_ok=ok, kernel=kernel)
    return res


def opt_run(Kmod, c, pas, inp, device, prec='f32'):
    """the finishing launch; a case that steps is also run in the fused form (opt_step(part=...)), which must give the same
    bits in every output"""
    res = _opt_once(Kmod, c, inp, device, False)
    if not c.norms_only:
        fused = _opt_once(Kmod, c, inp, device, True)
        for k in res:
            assert torch.equal(res[k]['out'], fused[k]['out']) and fused[k]['frame_ok'], \
                ('not reproducible: the fused form and the finishing launch differ', c, k)
    return res


def opt_coverage(seen):
    q = [(c, pl) for _, c, pl in seen]
    for kind in (OPT_RMSPROP, OPT_ADAM):
        st = [(c, pl) for c, pl in q if c.kind == kind and not c.norms_only]
        for n in OPT_SIZES:
            _need(('opt size', kind, n), (n in c.sizes for c, pl in st))
        _need(('opt host step', kind), (not c.stepdev for c, pl in st))
        _need(('opt device counter', kind), (c.stepdev for c, pl in st))
        for which in range(4):
            want = 'vec' if (which == 3 and kind == OPT_RMSPROP) else 'scalar'
            _need(('opt one pointer displaced alone', kind, which),
                  (any(n % 4 == 0 and sum(1 for v in d if v) == 1 and d[which] and sp == want
                       for n, d, sp in zip(c.sizes, c.disps, pl['spath'])) for c, pl in st))
        _need(('opt all aligned, 16-byte path', kind), (any(sp == 'vec' and n > OPT_STRIPE for n, sp in zip(c.sizes, pl['spath']))
                                                       for c, pl in st))
    _need('grad_norms scalar path by the gradient pointer alone', (any(n % 4 == 0 and p_ == 'scalar' for n, p_ in zip(c.sizes, pl['npath']))
                                                                   for c, pl in q))
    _need('one stripe exactly and one element more', (OPT_STRIPE in c.sizes and OPT_STRIPE + 1 in c.sizes for c, pl in q))
    _need('clip 0', (c.clip == 0.0 and not c.norms_only for c, pl in q))
    _need('clip above every norm', (c.clip >= 1e6 for c, pl in q))
    _need('clip below every norm', (c.clip == 1.0 and not c.norms_only and min(c.sizes) >= 256 for c, pl in q))
    _need('clip between the norms', (c.clip == 10.0 and not c.norms_only for c, pl in q))
    for gs in (1.0, 0.125):
        _need(('grad_scale', gs), (c.gs == gs and not c.norms_only for c, pl in q))
    for what, it in (('NaN, scalar path', (c.flag and c.flag[2] != c.flag[2] and pl['npath'][c.flag[0]] == 'scalar' for c, pl in q)),
                     ('NaN, vector path', (c.flag and c.flag[2] != c.flag[2] and pl['npath'][c.flag[0]] == 'vec' for c, pl in q)),
                     ('inf', (c.flag and c.flag[2] == float('inf') for c, pl in q)),
                     ('above 1e5 after grad_scale', (c.flag and 1e5 < c.flag[2] * c.gs < 1.0001e5 for c, pl in q)),
                     ('below 1e5 after grad_scale, above before', (c.flag and 1e5 > c.flag[2] * c.gs > 0.9999e5 for c, pl in q)),
                     ('none', (c.flag is None for c, pl in q))):
        _need(('flags', what), it)
    _need('exact sums of squares', (c.exact for c, pl in q))


FAMILIES['opt'] = Family(opt_cases, opt_plan, opt_inputs, opt_reference, opt_run, opt_coverage,
                         lambda c: (EXACT,) if c.exact else (REAL,))


# =====================================================================================================================
# 6. time moments
# =====================================================================================================================
def tm_cases():
    out = []

    def tc(B, C, L, lens, padfill=0, absent=(), zero_row=0, tight_row=0, hv='a', dv='o'):
        out.append(('tm B%d C%d L%d %s pad%d -%s%s%s' % (B, C, L, lens, padfill, '/'.join(absent), ' zero-row' if zero_row else '',
                                                         ' tight-row' if tight_row else ''),
                    Case(op='tm', B=B, C=C, L=L, lens=lens, padfill=padfill, absent=tuple(absent), zero_row=zero_row, tight_row=tight_row,
                         hv=hv, dv=dv)))
    tc(1, 1, 1, 'full', hv='c', dv='c')
    tc(1, 3, 7, 'full', absent=['gm'])
    tc(2, 2, 63, 'ragged', absent=['gs'], hv='o', dv='h')
    tc(5, 1, 64, 'ragged', padfill=1, absent=['gf'], hv='m', dv='a')
    tc(3, 3, 65, 'ragged', absent=['gm', 'gs'], hv='h', dv='m')
    tc(3, 3, 200, 'ragged', padfill=1)
    tc(2, 2, 64, 'full', zero_row=1)
    tc(2, 2, 64, 'full', tight_row=1, hv='o', dv='a')
    tc(3, 3, 200, 'ragged', absent=['gs', 'gf'], hv='c', dv='c')
    return out


def tm_plan(c, prec='f32'):
    return dict(kernel='time_moments_kernel', blocks=cdiv(c.B * c.C, 4), iters=cdiv(c.L, 64))


def tm_inputs(c, pas, seed):
    gen = _gen(seed)
    h = torch.randn(c.B, c.C, c.L, generator=gen)
    lens = torch.full((c.B,), c.L, dtype=torch.int64)
    if c.lens == 'ragged':
        lens = torch.tensor([(c.L, 1, max(1, c.L // 2), c.L - 1, 2)[b % 5] for b in range(c.B)], dtype=torch.int64)
    if not c.padfill:
        h = h * (torch.arange(c.L).view(1, 1, -1) < lens.view(-1, 1, 1)).float()
    if c.zero_row:
        h[0, 1] = 0.0
    if c.tight_row == 2:       # the same row without the grid.  NOT IN THE LIST: measured on the MI355X over ten draws, dh of this
        # row is off by 6e-6 .. 2e-4 of the scale (a single draw of the mean's rounding, amplified 1e4 times) and the fp32 CPU
        # model by 3e-7 .. 6e-5; two draws of ten miss the rule (once 33 x floor, once above 1e-4), m / s / f hold it always
        h[1, 0] = 100.0 + 0.01 * torch.randn(c.L, generator=gen)
    elif c.tight_row:          # mean 100, spread 2^-7 x [-3, 3] (0.01 in binary): offsets that sum to zero, so that fp32 holds
        offs = torch.randint(-3, 4, (c.L // 2,), generator=gen).float()              # the mean exactly
        h[1, 0] = 100.0 + torch.cat([offs, -offs])[torch.randperm(c.L, generator=gen)] * 2.0 ** -7
    g = lambda: torch.randn(c.B, c.C, generator=gen)  # noqa: E731
    return dict(h=h, lens=lens, gm=g(), gs=g(), gf=g())


def tm_reference(c, pas, inp, dtype, prec='f32'):
    """the contract above time_moments_fwd_kernel: the mean runs over ALL t; the s / f term of a row whose central moment is
    exactly zero is dropped from the gradient"""
    B, C, L = c.B, c.C, c.L
    h = inp['h'].to(dtype)
    mask = (torch.arange(L).view(1, 1, L) < inp['lens'].view(B, 1, 1)).to(dtype)
    lf = inp['lens'].view(B, 1, 1).to(dtype)
    cen = h - h.sum(2, keepdim=True) / lf * mask
    s2, s4 = (cen ** 2).sum(2, keepdim=True), (cen ** 4).sum(2, keepdim=True)
    a1, a3 = (cen * mask).sum(2, keepdim=True), (cen ** 3 * mask).sum(2, keepdim=True)
    z = torch.zeros(B, C, 1, dtype=dtype)
    gm, gs, gf = [(inp[k].to(dtype).view(B, C, 1) if k not in c.absent else z) for k in ('gm', 'gs', 'gf')]
    one = torch.ones_like(s2)
    ks = torch.where(s2 > 0, gs / (lf * torch.where(s2 > 0, s2, one).sqrt()), z)
    kf = torch.where(s4 > 0, gf / (lf * torch.where(s4 > 0, s4, one) ** 0.75), z)
    out = dict(m=(h.sum(2, keepdim=True) / lf).view(B, C), s=(s2.sqrt() / lf).view(B, C), f=(s4 ** 0.25 / lf).view(B, C),
               dh=gm / lf + ks * (cen - a1 / lf) + kf * (cen ** 3 - a3 / lf))
    return dict(out, _bit=('m', 's', 'f', 'dh') if L == 1 else ())      # one step: m = h, s = f = 0, dh = gm - no rounding anywhere


def tm_run(Kmod, c, pas, inp, device, prec='f32'):
    B, C, L = c.B, c.C, c.L
    h = place(inp['h'], c.hv, device)
    lens = inp['lens'].to(device)
    frames = dict((k, FlatFrame((B, C), device, nan(B, C))) for k in ('m', 's', 'f'))
    Kmod.time_moments_fwd(h, lens, frames['m'].win, frames['s'].win, frames['f'].win)
    frames['dh'] = Frame(B, C, L, c.dv, device, nan(B, C, L))
    g = [(inp[k].to(device) if k not in c.absent else None) for k in ('gm', 'gs', 'gf')]
    Kmod.time_moments_bwd(h, lens, g[0], g[1], g[2], frames['dh'].win)
    return results(frames, 'time_moments_kernel')


def tm_coverage(seen):
    q = [c for _, c, pl in seen]
    for L in (1, 7, 63, 64, 65, 200):
        _need(('tm L', L), (c.L == L for c in q))
    for bc in (1, 3, 4, 5, 9):
        _need(('tm B x C', bc), (c.B * c.C == bc for c in q))
    _need('tm slab views of different pitch', (c.hv != c.dv and 'c' not in (c.hv, c.dv) for c in q))
    for lens in ('full', 'ragged'):
        _need(('tm lens', lens), (c.lens == lens for c in q))
    for pf in (0, 1):
        _need(('tm padded steps non-zero', pf), (c.padfill == pf and c.lens == 'ragged' for c in q))
    for k in ('gm', 'gs', 'gf'):
        _need(('tm absent alone', k), (c.absent == (k,) for c in q))
    _need('tm two absent', (len(c.absent) == 2 for c in q))
    _need('tm all-zero row', (c.zero_row for c in q))
    _need('tm mean 100, spread 0.01', (c.tight_row for c in q))


FAMILIES['tm'] = Family(tm_cases, tm_plan, tm_inputs, tm_reference, tm_run, tm_coverage, _real)


# =====================================================================================================================
# 7. transposes and conversions: bct_to_tbc, tbc_to_bct, to_bf16
# =====================================================================================================================
BF = torch.bfloat16
TIES = [1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 2.0 ** -7 + 2.0 ** -8),       # to even: down, up
        0.0, -0.0, 3.3895313892515355e38, 3.4028234663852886e38, -3.4028234663852886e38,     # largest bf16; rounds past it
        1e-40, -1e-40, 2.0 ** -149, 2.0 ** -134 + 2.0 ** -142, float('inf'), -float('inf')]   # subnormals (one a tie), infinities


def tr_cases():
    out = []
    for B, Cc, T in ((1, 1, 1), (1, 31, 33), (3, 32, 32), (1, 33, 31), (3, 70, 1), (1, 1, 70), (3, 70, 70), (1, 32, 70)):
        for i16 in (0, 1):
            for o16 in (0, 1):
                for op in ('bct_to_tbc', 'tbc_to_bct'):
                    out.append(('%s B%d C%d T%d %d%d' % (op, B, Cc, T, i16, o16), Case(op=op, B=B, Cc=Cc, T=T, i16=i16, o16=o16,
                                                                                      pitched=int(op == 'bct_to_tbc' and Cc != 32))))
    for shape, pitched in (((7, 33), 1), ((1000,), 0), ((257,), 0), ((3, 5, 7), 0), ((1, 70), 1)):
        out.append(('to_bf16 %s%s' % ('x'.join(map(str, shape)), ' pitched' if pitched else ''),
                    Case(op='to_bf16', shape=shape, pitched=pitched, i16=0, o16=1)))
    return out


def tr_plan(c, prec='f32'):
    if c.op == 'to_bf16':
        return dict(kernel='to_bf16_2d_kernel', narrowing=True)
    R, cols = (c.Cc, c.T) if c.op == 'bct_to_tbc' else (c.T, c.Cc)
    return dict(kernel='transpose_batched_kernel<%d,%d>' % (c.i16, c.o16), tiles=(cdiv(cols, 32), cdiv(R, 32)),
                narrowing=bool(c.o16 and not c.i16))


def tr_inputs(c, pas, seed):
    gen = _gen(seed)
    shape = c.shape if c.op == 'to_bf16' else ((c.B, c.Cc, c.T) if c.op == 'bct_to_tbc' else (c.T, c.B, c.Cc))
    x = torch.randn(*shape, generator=gen)
    flat = x.view(-1)
    if flat.numel() > len(TIES):
        flat[1:1 + len(TIES)] = torch.tensor(TIES)
    else:
        flat.copy_(torch.tensor(TIES[:flat.numel()]) if flat.numel() > 1 else torch.tensor([TIES[1]]))
    return dict(x=x.bfloat16() if c.i16 else x)


def tr_reference(c, pas, inp, dtype, prec='f32'):
    x = inp['x']
    if c.op == 'bct_to_tbc':
        x = x.permute(2, 0, 1)
    elif c.op == 'tbc_to_bct':
        x = x.permute(1, 2, 0)
    return dict(y=x.contiguous().float().to(dtype), _bit=('y',))


def tr_run(Kmod, c, pas, inp, device, prec='f32'):
    x, kernel = inp['x'], tr_plan(c)['kernel']
    odt = BF if c.o16 else torch.float32
    if c.pitched:                           # a block of a wider slab: rows at a pitch, a batch stride with rows around
        shp = (1,) + tuple(x.shape) if x.dim() == 2 else tuple(x.shape)
        slab = torch.full((shp[0], shp[1] + 2, shp[2] + 5), 99.0, dtype=x.dtype, device=device)
        xin = slab[:, 1:shp[1] + 1, 2:shp[2] + 2]
        xin.copy_(x.view(shp))
        xin = xin[0] if x.dim() == 2 else xin
    else:
        xin = in_flat(x, device)
    if c.op == 'to_bf16':
        fr = FlatFrame(tuple(c.shape), device, nan(*c.shape), dtype=BF)
        Kmod.to_bf16(xin, out=fr.win)
    elif c.op == 'bct_to_tbc':
        fr = FlatFrame((c.T, c.B, c.Cc), device, nan(c.T, c.B, c.Cc), dtype=odt)
        Kmod.bct_to_tbc(xin, out=fr.win)
    else:
        fr = FlatFrame((c.B, c.Cc, c.T), device, nan(c.B, c.Cc, c.T), dtype=odt)
        Kmod.tbc_to_bct(xin, out=fr.win)
    return results(dict(y=fr), kernel)


def tr_coverage(seen):
    for op in ('bct_to_tbc', 'tbc_to_bct'):
        q = [(c, pl) for _, c, pl in seen if c.op == op]
        for i16 in (0, 1):
            for o16 in (0, 1):
                for n in (1, 31, 32, 33, 70):
                    _need((op, i16, o16, 'R / Cc', n), (c.i16 == i16 and c.o16 == o16 and n in (c.Cc, c.T) for c, pl in q))
                _need((op, i16, o16, 'ragged tiles on both axes'), (c.i16 == i16 and c.o16 == o16 and pl['tiles'] == (3, 3) for c, pl in q))
        for B in (1, 3):
            _need((op, 'B', B), (c.B == B for c, pl in q))
    _need('bct_to_tbc pitched input', (c.pitched and c.op == 'bct_to_tbc' for _, c, pl in seen))
    _need('to_bf16 pitched rows', (c.pitched and c.op == 'to_bf16' for _, c, pl in seen))
    _need('to_bf16 any contiguous tensor', (not c.pitched and c.op == 'to_bf16' and len(c.shape) == 3 for _, c, pl in seen))
    assert len(TIES) == 15


FAMILIES['tr'] = Family(tr_cases, tr_plan, tr_inputs, tr_reference, tr_run, tr_coverage, _real)


# =====================================================================================================================
# 8. one-output Linear and column sums: rowdot_fwd, rowdot_bwd, col_sum
# =====================================================================================================================
RD_ROWS = 64
SMALL_WS = 1 << 17


def rd_cases():
    out = []

    def rc(M, K, form, **kw):
        d = dict(op='rowdot', M=M, K=K, form=form, bias=1, ycol=0, gate=0, dx=1, dw=1, acc=0, x16=0)
        d.update(kw)
        out.append(('rowdot M%d K%d %s %s' % (M, K, form, ' '.join('%s%d' % (k, v) for k, v in sorted(kw.items()))), Case(**d)))
    rc(1, 1, 'k%4'); rc(3, 3, 'k%4', bias=0, gate=1); rc(4, 4, 'vec', ycol=1); rc(5, 255, 'k%4', acc=1, gate=1)
    rc(63, 256, 'vec', gate=1, acc=1); rc(64, 257, 'k%4', dx=0); rc(65, 512, 'vec', dw=0, ycol=1); rc(130, 1028, 'vec', gate=1, bias=0)
    rc(5, 256, 'ldx', gate=1); rc(5, 256, 'xbase'); rc(5, 256, 'wbase', acc=1); rc(130, 512, 'ldx', ycol=1, acc=1)
    rc(64, 256, 'vec', dx=0, dw=0)
    rc(65, 257, 'x16', x16=1, gate=1); rc(4, 1028, 'x16', x16=1, acc=1, ycol=1); rc(130, 256, 'x16', x16=1, bias=0, dx=0)

    def cs(M, N, **kw):
        d = dict(op='col_sum', M=M, N=N, acc=0, defer=0, x16=0, xv='a')
        d.update(kw)
        out.append(('col_sum M%d N%d %s' % (M, N, ' '.join('%s%s' % (k, v) for k, v in sorted(kw.items()))), Case(**d)))
    cs(1, 1, xv='c'); cs(16, 63, acc=1); cs(17, 64, xv='o'); cs(64, 65, acc=1, defer=1); cs(1000, 200, defer=2, xv='h')
    cs(1000, 1, acc=1); cs(17, 200, x16=1); cs(16, 200, x16=1, acc=1); cs(64, 63, defer=2, acc=1, xv='m')
    return out


def rd_plan(c, prec='f32'):
    if c.op == 'col_sum':
        gx = cdiv(c.N, 64)
        gy = max(1, min(cdiv(1024, gx), cdiv(c.M, 16)))
        ws = min(SMALL_WS, 64 * c.N) if c.M > 16 else 0
        gy = min(gy, ws // c.N) if gy > 1 and ws >= 2 * c.N else 1
        gy = cdiv(c.M, cdiv(c.M, gy))
        return dict(kernel='col_sum_kernel', split=gy > 1, gy=gy, twice=gy > 1)
    path = 'bf16 storage' if c.x16 else ('vec' if c.form == 'vec' else 'scalar')
    pitch, off, woff = rd_geom(c)
    if not c.x16:       # the kernel's own condition, on the geometry the runner builds
        assert (path == 'vec') == (c.K % 4 == 0 and pitch % 4 == 0 and off % 4 == 0 and woff % 4 == 0), c
    return dict(kernel='rowdot_kernel %s' % path, path=path, ktiles=cdiv(c.K, 256), mblocks=cdiv(c.M, RD_ROWS),
                ws=cdiv(c.M, RD_ROWS) * (c.K + 1), twice=bool(c.dw), pitch=pitch, off=off, woff=woff)


def rd_geom(c):
    """(row pitch of x, offset of x and of w in floats from a 16-byte aligned address): every refusal of the 16-byte path
    ALONE - 'k%4' on an aligned base with a pitch % 4 == 0, 'ldx' with K % 4 == 0 on an aligned base, and so on"""
    K = c.K
    al = roundup(K, 4) + 4
    return dict(vec=(al, 0, 0), ldx=(K + 2, 0, 0), xbase=(al, 1, 0), wbase=(al, 0, 1), x16=(K + 5, 2, 0))[c.form] if c.form != 'k%4' \
        else (al, 0, 0)


def rd_inputs(c, pas, seed):
    gen = _gen(seed)
    d = _draw(pas, gen)
    if c.op == 'col_sum':
        X = d(c.M, c.N)
        if pas is REAL:
            X = X / c.M ** 0.5
        return dict(X=X.bfloat16() if c.x16 else X, out0=d(c.N))
    x = d(c.M, c.K)
    if c.gate and c.K >= 3:
        x[:, 1], x[0, 2] = 0.0, -0.0              # exact zeros: the gate's convention is x > 0
    w = d(c.K)
    if pas is REAL:
        w = w / c.K ** 0.5
    return dict(x=x.bfloat16() if c.x16 else x, w=w, bias=d(1), dy=d(c.M), dwb0=d(c.K + 1))


def rd_reference(c, pas, inp, dtype, prec='f32'):
    if c.op == 'col_sum':
        s = inp['X'].to(dtype).sum(0)
        return dict(out=s + inp['out0'].to(dtype) if c.acc else s)
    rb = prec == 'bf16' or c.x16
    r = rnd16 if rb else (lambda t: t)
    x, w, dy = r(inp['x'].float()).to(dtype), r(inp['w']).to(dtype), inp['dy'].to(dtype)
    y = (x * w.view(1, -1)).sum(1)
    out = dict(y=y + inp['bias'].to(dtype)[0] if c.bias else y)
    g = r(inp['dy']).to(dtype).view(-1, 1)
    slope = f32(pas['slope'])
    if c.dx:
        dv = g * w.view(1, -1)
        if c.gate:
            dv = torch.where(inp['x'].float() > 0, dv, dv * slope)
        out['dx'] = dv
    if c.dw:
        dwb = torch.cat([(g * x).sum(0), dy.sum().view(1)])          # (db sums the unrounded dy)
        out['dwb'] = dwb + inp['dwb0'].to(dtype) if c.acc else dwb
    return out


def rd_run(Kmod, c, pas, inp, device, prec='f32'):
    pl = rd_plan(c, prec)
    if c.op == 'col_sum':
        fr = FlatFrame((c.N,), device, inp['out0'] if c.acc else nan(c.N))
        if c.x16:
            slab = torch.full((c.M + 2, c.N + 6), 99.0, dtype=BF, device=device)
            X = slab[1:c.M + 1, 2:c.N + 2]
            X.copy_(inp['X'])
        else:
            X = in2(inp['X'], c.xv, device) if c.xv != 'c' else in_flat(inp['X'], device)
        if c.defer == 0:
            Kmod.col_sum(X, fr.win, accumulate=bool(c.acc))
        else:
            with Kmod.deferred_reduces():
                Kmod.col_sum(X, fr.win, accumulate=bool(c.acc), defer=c.defer == 1)
                early = fr.window() if c.defer == 2 else None            # defer=False: complete inside the scope
            assert early is None or torch.equal(early.view(torch.int32), fr.window().view(torch.int32)), \
                ('col_sum(defer=False) was not complete inside the recording scope', c)
        return results(dict(out=fr), pl['kernel'])
    M, K = c.M, c.K
    dt = BF if c.x16 else torch.float32
    pitch, off, woff = rd_geom(c)
    if c.x16:
        slab = torch.full((M + 2, K + 5), 99.0, dtype=BF, device=device)
        x = slab[1:M + 1, 2:K + 2]
        x.copy_(inp['x'])
    else:
        x = StridedFrame((M, K), (pitch, 1), off, device, inp['x'], sentinel=99.0).win
    w = in_flat(inp['w'], device, off=woff)
    frames = {}
    frames['y'] = StridedFrame((M,), (2,), 1, device, nan(M)) if c.ycol else FlatFrame((M,), device, nan(M))
    Kmod.rowdot_fwd(x, w, inp['bias'].to(device) if c.bias else None, frames['y'].win)
    dy = StridedFrame((M,), (2,), 0, device, inp['dy'], sentinel=99.0).win if c.ycol else in_flat(inp['dy'], device)
    dx = None
    if c.dx:
        if c.x16:
            frames['dx'] = FlatFrame((M, K), device, nan(M, K), dtype=BF)
            dx = frames['dx'].win
        else:
            frames['dx'], dx = out2(M, K, 'o', device, nan(M, K))
    dw = db = None
    if c.dw:
        frames['dwb'] = FlatFrame((K + 1,), device, inp['dwb0'] if c.acc else nan(K + 1))
        dw, db = frames['dwb'].win[:K], frames['dwb'].win[K:]
    Kmod.rowdot_bwd(dy, x, w, dx=dx, dw=dw, db=db, gate=bool(c.gate), slope=pas['slope'], accumulate=bool(c.acc))
    return results(frames, pl['kernel'])


def rd_coverage(seen):
    q = [(c, pl) for _, c, pl in seen if c.op == 'rowdot']
    for M in (1, 3, 4, 5, 63, 64, 65, 130):
        _need(('rowdot M', M), (c.M == M for c, pl in q))
    for K in (1, 3, 4, 255, 256, 257, 512, 1028):
        _need(('rowdot K', K), (c.K == K for c, pl in q))
    _need('rowdot 16-byte path', (c.form == 'vec' and c.K % 4 == 0 for c, pl in q))
    for K in (1, 3, 255, 257):
        _need(('rowdot refusal alone: K % 4', K), (c.K == K and pl['pitch'] % 4 == 0 and pl['off'] == 0 and pl['woff'] == 0 and
                                                   pl['path'] == 'scalar' and not c.x16 for c, pl in q))
    _need('rowdot refusal alone: ldx % 4', (c.K % 4 == 0 and pl['pitch'] % 4 and pl['off'] == 0 and pl['woff'] == 0 and pl['path'] == 'scalar'
                                            for c, pl in q))
    _need('rowdot refusal alone: base of x', (c.K % 4 == 0 and pl['pitch'] % 4 == 0 and pl['off'] % 4 and pl['woff'] == 0 and
                                              pl['path'] == 'scalar' for c, pl in q))
    _need('rowdot refusal alone: base of w', (c.K % 4 == 0 and pl['pitch'] % 4 == 0 and pl['off'] == 0 and pl['woff'] % 4 and
                                              pl['path'] == 'scalar' for c, pl in q))
    _need('rowdot second K tile with a ragged edge', (pl['ktiles'] == 2 and c.K % 256 for c, pl in q))
    _need('rowdot several row blocks', (pl['mblocks'] == 3 for c, pl in q))
    for k in ('ycol', 'gate', 'acc', 'x16', 'bias', 'dx', 'dw'):
        for v in (0, 1):
            _need(('rowdot', k, v), (c[k] == v for c, pl in q))
    _need('rowdot nothing but dx absent and dw absent', (not c.dx and not c.dw for c, pl in q))
    s = [(c, pl) for _, c, pl in seen if c.op == 'col_sum']
    for M in (1, 16, 17, 64, 1000):
        _need(('col_sum M', M), (c.M == M for c, pl in s))
    for N in (1, 63, 64, 65, 200):
        _need(('col_sum N', N), (c.N == N for c, pl in s))
    for split in (False, True):
        for acc in (0, 1):
            _need(('col_sum split / accumulate', split, acc), (pl['split'] == split and c.acc == acc for c, pl in s))
    for d in (0, 1, 2):
        _need(('col_sum defer', d), (c.defer == d and pl['split'] for c, pl in s))
    _need('col_sum pitched', (c.xv != 'c' for c, pl in s))
    _need('col_sum bf16 storage, both forms', (c.x16 and pl['split'] for c, pl in s))


FAMILIES['rd'] = Family(rd_cases, rd_plan, rd_inputs, rd_reference, rd_run, rd_coverage, _both)


# =====================================================================================================================
# 1. weight norm: one launch over a table of tensors
# =====================================================================================================================
WN_FILL = 77.0
# (shape of v, stride, pad, outputs present, accumulate in the backward)
WN_TABLE = [
    ((130,), 1, 0, 'w', 0),                 # 1-D: 130 rows of one column - dv is analytically zero
    ((1, 63), 1, 0, 'w', 1),
    ((3, 64), 1, 0, 'w', 0),
    ((4, 65), 1, 0, 'w', 1),
    ((5, 129), 1, 0, 'w', 0),
    ((5, 9, 7), 2, 3, 'w a b', 1),          # cols 63; aligned scatter
    ((33, 3, 3), 1, 1, 'a', 0),             # rows % 32, odd d1; w absent
    ((3, 5, 1), 1, 0, 'w b', 1),            # K 1; wpa absent
    ((4, 3, 8), 4, 2, 'w a b', 0),          # k = 2 s: the shifted phases would need a third slot - not aligned
    ((7, 3, 9), 4, 3, 'w b', 0),            # aligned, shift by pad % s
    ((6, 5, 17), 8, 4, 'a b', 1),           # aligned at stride 8
    ((2, 4, 8), 4, 4, 'w a', 0),            # pad % s == 0; wpb absent
    ((3, 3, 7), 2, 2, 'w a b', 1),          # stride 2, not aligned
]


def wn_cases():
    return [('table of %d' % len(WN_TABLE), Case(op='wn', table=WN_TABLE)),
            ('one bias', Case(op='wn', table=[((1,), 1, 0, 'w', 0)])),
            ('one row of 64', Case(op='wn', table=[((1, 64), 1, 0, 'w', 1)]))]


def _wn_dims(shape):
    rows = shape[0]
    cols = 1
    for n in shape[1:]:
        cols *= n
    d1, K = (shape[1], shape[2]) if len(shape) == 3 else (cols, 1)
    return rows, cols, d1, K


def scatter_shift(s, pad, r):
    qmax = (pad + s - 1) // s
    return qmax - ((pad - r + s - 1) // s if pad > r else 0)


def scatter_aligned(K, s, pad):
    """common.h ag_scatter_aligned, restated"""
    if s <= 1 or pad % s == 0:
        return False
    mt = cdiv(K, s)
    return all(((K - r + s - 1) // s if r < K else 0) + scatter_shift(s, pad, r) <= mt for r in range(s))


def wn_plan(c, prec='f32'):
    mr = max(e[0][0] for e in c.table)
    ent = []
    for shape, s, pad, has, acc in c.table:
        rows, cols, d1, K = _wn_dims(shape)
        ent.append(dict(rows=rows, cols=cols, d1=d1, K=K, s=s, pad=pad, has=has.split(), acc=acc, dim=len(shape),
                        aligned=scatter_aligned(K, s, pad), surplus=cdiv(rows, 4) < cdiv(mr, 4)))
    return dict(kernel='weight_norm_kernel', max_rows=mr, entries=ent)


def wn_inputs(c, pas, seed):
    gen = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    return [dict(v=r(*e[0]), g=r(e[0][0]), dw=r(*e[0]), dv0=r(*e[0]), dg0=r(e[0][0])) for e in c.table]


def wn_reference(c, pas, inp, dtype, prec='f32'):
    out, scale, bit = {}, {}, []
    for i, (e, t) in enumerate(zip(wn_plan(c)['entries'], inp)):
        v, g, dw = [t[k].to(dtype).reshape(e['rows'], -1) for k in ('v', 'g', 'dw')]
        inv = 1.0 / (v * v).sum(1, keepdim=True).sqrt()
        w = v * (g * inv)
        for k in e['has']:
            out['%s.%d' % (dict(w='w', a='wpa', b='wpb')[k], i)] = w
        if 'a' in e['has'] or 'b' in e['has']:
            out['placed.%d' % i] = torch.ones(1, dtype=torch.int32)        # every layout holds the very value stored as w
            out['image.%d' % i] = torch.ones(1, dtype=torch.int32)         # bf16 image = RNE of the fp32 value beside it
        dot = (v * dw).sum(1, keepdim=True)
        dg, dv = dot * inv, g * inv * (dw - v * dot * inv * inv)
        if e['cols'] == 1:
            # a one-element row: w = g sign(v), dv is identically zero; the error is taken as a fraction of |g / v| |dw|,
            # the size of the two terms that cancel
            dv = torch.zeros_like(dv)
            scale['dv.%d' % i] = float((g / v * dw).abs().max()) + (float(t['dv0'].abs().max()) if e['acc'] else 0.0)
        if e['acc']:
            dg, dv = dg + t['dg0'].to(dtype).view(-1, 1), dv + t['dv0'].to(dtype).reshape(e['rows'], -1)
        out['dv.%d' % i], out['dg.%d' % i] = dv, dg.view(-1)
    return dict(out, _scale=scale, _bit=tuple(bit))


def _wq_index(ch, tap, row, taps, mpad):
    return ((((ch >> 4) * taps + tap) * 2 + ((ch >> 3) & 1)) * mpad + row) * 8 + (ch & 7)


def wn_maps(e):
    """per layout: (fp32 numel, index [rows, cols] of every element of v in the fp32 layout, index in the bf16 image)"""
    rows, d1, K, s = e['rows'], e['d1'], e['K'], e['s']
    r = torch.arange(rows).view(rows, 1, 1)
    o = torch.arange(d1).view(1, d1, 1)
    k = torch.arange(K).view(1, 1, K)
    d0p = roundup(rows, 32)
    ia = ((o * K + k) * d0p + r).reshape(rows, -1)
    qa = _wq_index(o, k, r, K, d0p).reshape(rows, -1)
    mt, mp = cdiv(K, s), roundup(d1 * s, 32)
    sh = torch.tensor([scatter_shift(s, e['pad'], int(kk) % s) if e['aligned'] else 0 for kk in range(K)]).view(1, 1, K)
    m, rr = k // s + sh, k % s
    ib = ((r * mt + m) * mp + o * s + rr).reshape(rows, -1)
    qb = _wq_index(r + 0 * o, m + 0 * o, o * s + rr + 0 * r, mt, mp).reshape(rows, -1)
    na, nb = roundup(d1, 2) * K * d0p, roundup(rows, 2) * mt * mp
    # what ag_wpa_numel / ag_wpb_numel give: the fp32 layout and behind it its bf16 image, channels rounded up to 16
    return dict(a=(na, ia, qa), b=(nb, ib, qb), total_a=na + roundup(d1, 16) * K * d0p // 2, total_b=nb + roundup(rows, 16) * mt * mp // 2)


def _layout_facts(fr, n32, idx, q, wvals):
    """of a prepared layout after the call: (values at the written slots [rows, cols], pad slots of the fp32 layout and of
    the bf16 image as they were, the slots bit-equal to `wvals`, the image = RNE of the fp32 value beside it)"""
    buf = fr.window().view(-1)
    vals = buf[idx]
    a16, b16 = buf.clone().view(torch.int16), torch.full_like(buf, WN_FILL).view(torch.int16)
    img = buf.numel() > n32
    for t in (a16, b16):
        t[2 * idx.reshape(-1)] = 0
        t[2 * idx.reshape(-1) + 1] = 0
        if img:
            t[2 * n32 + q.reshape(-1)] = 0
    rest = torch.equal(a16, b16)
    placed = wvals is None or torch.equal(vals.view(torch.int32), wvals.view(torch.int32))
    image = (not img) or torch.equal(buf.view(torch.int16)[2 * n32 + q], vals.bfloat16().view(torch.int16))
    return vals, rest, placed, image


def wn_run(Kmod, c, pas, inp, device, prec='f32'):
    pl = wn_plan(c)
    frames, fwd, bwd, res = {}, [], [], {}
    for i, (e, t) in enumerate(zip(pl['entries'], inp)):
        v, g = in_flat(t['v'], device), in_flat(t['g'], device)
        ent = dict(v=v, g=g, stride=e['s'], pad=e['pad'])
        if 'w' in e['has']:
            frames['w.%d' % i] = FlatFrame(tuple(t['v'].shape), device, nan(*t['v'].shape))
            ent['w'] = frames['w.%d' % i].win
        for k, numel in (('a', lambda: Kmod.wpa_numel(e['rows'], e['d1'], e['K'])), ('b', lambda: Kmod.wpb_numel(e['rows'], e['d1'], e['K'], e['s']))):
            if k in e['has']:
                n = numel()
                frames['wp%s.%d' % (k, i)] = FlatFrame((n,), device, torch.full((n,), WN_FILL))
                ent['wp' + k] = frames['wp%s.%d' % (k, i)].win
        fwd.append(ent)
        dvf = FlatFrame(tuple(t['v'].shape), device, t['dv0'] if e['acc'] else nan(*t['v'].shape))
        dgf = FlatFrame((e['rows'],), device, t['dg0'] if e['acc'] else nan(e['rows']))
        frames['dv.%d' % i], frames['dg.%d' % i] = dvf, dgf
        bwd.append(dict(v=v, g=g, dw=in_flat(t['dw'], device), dv=dvf.win, dg=dgf.win, accumulate=bool(e['acc'])))
    Kmod.weight_norm_fwd(fwd)
    Kmod.weight_norm_bwd(bwd)
    kernel = pl['kernel']
    for i, e in enumerate(pl['entries']):
        maps = wn_maps(e)
        wv = frames['w.%d' % i].window().reshape(e['rows'], -1) if 'w' in e['has'] else None
        placed = image = True
        for k in ('a', 'b'):
            name = 'wp%s.%d' % (k, i)
            if k not in e['has']:
                continue
            fr = frames.pop(name)
            n32, idx, q = maps[k]
            assert fr.n >= n32, 'the layout is smaller than its fp32 part'
            vals, rest, p_, im = _layout_facts(fr, n32, idx, q, wv)
            if wv is None:
                wv = vals                               # w absent: the two layouts must at least agree with each other
            placed, image = placed and p_, image and im
            res[name] = dict(out=vals, frame_ok=fr.untouched() and rest, kernel=kernel)
        if 'a' in e['has'] or 'b' in e['has']:
            res['placed.%d' % i] = dict(out=torch.tensor([int(placed)], dtype=torch.int32), frame_ok=True, kernel=kernel)
            res['image.%d' % i] = dict(out=torch.tensor([int(image)], dtype=torch.int32), frame_ok=True, kernel=kernel)
    res.update(results(frames, kernel))
    return res


def wn_coverage(seen):
    ent = [e for _, c, pl in seen for e in pl['entries']]
    big = [e for _, c, pl in seen if len(pl['entries']) > 1 for e in pl['entries']]
    for rows in (1, 3, 4, 5, 130):
        _need(('wn rows in one table', rows), (e['rows'] == rows for e in big))
    for cols in (1, 63, 64, 65, 129):
        _need(('wn cols', cols), (e['cols'] == cols for e in ent))
    for dim in (1, 2, 3):
        _need(('wn v.dim()', dim), (e['dim'] == dim for e in ent))
    for K in (1, 3, 7):
        _need(('wn K', K), (e['K'] == K and e['dim'] == 3 for e in ent))
    for s in (1, 2, 4, 8):
        _need(('wn stride', s), (e['s'] == s and 'b' in e['has'] for e in ent))
    for al in (False, True):
        _need(('wn aligned scatter layout', al), (e['aligned'] == al and 'b' in e['has'] and e['s'] > 1 and e['pad'] > 0 for e in ent))
    _need('wn pad % s == 0 with a layout', (e['s'] > 1 and e['pad'] and e['pad'] % e['s'] == 0 for e in ent))
    _need('wn odd d1', (e['d1'] % 2 and 'a' in e['has'] for e in ent))
    _need('wn rows % 32 (both layouts padded)', (e['rows'] % 32 and (e['d1'] * e['s']) % 32 and 'a' in e['has'] and 'b' in e['has'] for e in ent))
    for k in ('w', 'a', 'b'):
        _need(('wn absent', k), (e['dim'] == 3 and k not in e['has'] for e in ent))
    for acc in (0, 1):
        _need(('wn backward accumulate', acc), (e['acc'] == acc for e in ent))
    _need('wn surplus blocks of a short tensor', (e['surplus'] for e in big))
    _need('wn a table of one', (len(pl['entries']) == 1 for _, c, pl in seen))
    _need('wn one-element rows: dv cancels to zero', (e['cols'] == 1 and not e['acc'] for e in ent))


FAMILIES['wn'] = Family(wn_cases, wn_plan, wn_inputs, wn_reference, wn_run, wn_coverage, _real)


# =====================================================================================================================
# 9. Conv2DLSTM pieces and layer norm on [H, B, F, W] maps
# =====================================================================================================================
CL_SHAPES = ((1, 2, 1, 1), (3, 2, 4, 16), (3, 1, 5, 37), (1, 2, 5, 16), (3, 2, 1, 37))
CL_BIG = (3, 2, 16, 11000)                  # 1 056 000 elements: the second grid-stride round
CL_IN = dict(peep_fwd=('y:y4', 'c:m', 'wci:p', 'wcf:p'), peep_bwd=('dj:m', 'di:m', 'df:m', 'do:m', 'c:m', 'wci:p', 'wcf:p', 'dc0:m'),
             cell_fwd=('j:m', 'i:m', 'f:m', 'c:m', 'o:m', 'wco:p'), cell_bwd=('j:m', 'i:m', 'f:m', 'c:m', 'cn:m', 'wco:p', 'dcn0:m', 'dop:m'),
             out_fwd=('o:m', 'c:m'), out_bwd=('o:m', 'c:m', 'dh:m'))


def cl_cases():
    out = []

    def cc(op, shape, absent=(), fb=0.0):
        out.append(('%s %s -%s fb%g' % (op, 'x'.join(map(str, shape)), '/'.join(absent), fb),
                    Case(op=op, shape=tuple(shape), absent=tuple(absent), fb=fb)))
    S = CL_SHAPES
    cc('peep_fwd', S[0]); cc('peep_fwd', S[1], ['wci']); cc('peep_fwd', S[2], ['wcf']); cc('peep_fwd', S[3], ['wci', 'wcf'])
    cc('peep_fwd', S[4]); cc('peep_fwd', CL_BIG)
    cc('peep_bwd', S[0]); cc('peep_bwd', S[1], ['wci', 'dwci']); cc('peep_bwd', S[2], ['wcf', 'dwcf']); cc('peep_bwd', S[3], ['dwci'])
    cc('peep_bwd', S[4], ['dwcf']); cc('peep_bwd', S[1], ['wci', 'wcf', 'dwci', 'dwcf']); cc('peep_bwd', CL_BIG)
    cc('cell_fwd', S[0], fb=1.0); cc('cell_fwd', S[1]); cc('cell_fwd', S[2], ['wco'], fb=1.0); cc('cell_fwd', S[3]); cc('cell_fwd', S[4], fb=1.0)
    cc('cell_fwd', CL_BIG, fb=1.0)
    cc('cell_bwd', S[0]); cc('cell_bwd', S[1], fb=1.0); cc('cell_bwd', S[2], ['dwco']); cc('cell_bwd', S[3], ['wco', 'dwco'], fb=1.0)
    cc('cell_bwd', S[4], fb=1.0); cc('cell_bwd', CL_BIG)
    for s in (S[0], S[1], S[2], CL_BIG):
        cc('out_fwd', s); cc('out_bwd', s)

    def ln(H, B, F, W, eps=1e-12, special=''):
        out.append(('layer_norm %dx%dx%dx%d eps%g %s' % (H, B, F, W, eps, special),
                    Case(op='ln', shape=(H, B, F, W), eps=eps, special=special, absent=(), fb=0.0)))
    ln(1, 2, 1, 1); ln(3, 2, 4, 8); ln(1, 2, 5, 51, eps=1e-5); ln(1, 2, 4, 64); ln(1, 2, 1, 257, eps=1e-5); ln(1, 2, 300, 10)
    ln(3, 1, 4, 8, special='const'); ln(3, 1, 4, 8, eps=1e-5, special='const'); ln(3, 2, 4, 8, special='mean1000'); ln(3, 2, 4, 8, special='mean1000 plain')
    return out


def cl_plan(c, prec='f32'):
    H, B, F, W = c.shape
    n = H * B * F * W
    if c.op == 'ln':
        return dict(kernel='layer_norm_hbfw_kernel', sample=H * F * W, iters=cdiv(H * F * W, 256), fiters=cdiv(F, 256), rounds=1)
    return dict(kernel='convlstm_%s_kernel' % c.op, rounds=_rounds(n), sample=0)


def _cl_shape(kind, shape):
    H, B, F, W = shape
    return dict(m=(H, B, F, W), y4=(H, B, 4 * F, W), p=(H, F, W))[kind]


def cl_inputs(c, pas, seed):
    gen = _gen(seed)
    d = _draw(pas, gen)
    H, B, F, W = c.shape
    if c.op != 'ln':
        return dict((s.split(':')[0], d(*_cl_shape(s.split(':')[1], c.shape))) for s in CL_IN[c.op])
    x = d(H, B, F, W)
    if c.special == 'const':
        x.fill_(3.0)
    elif c.special == 'mean1000 plain':    # the same without the grid: the mean's own rounding is in (measured: within the rule)
        x = 1000.0 + d(H, B, F, W)
    elif c.special == 'mean1000':          # mean 1000, spread 1: offsets per sample that sum to zero, so fp32 holds the mean
        for b in range(B):
            offs = torch.randint(-3, 4, (H * F * W // 2,), generator=gen).float()
            x[:, b] = 1000.0 + torch.cat([offs, -offs])[torch.randperm(H * F * W, generator=gen)].view(H, F, W)
    xd = x.double()
    m = xd.mean(dim=(0, 2, 3))
    r = 1.0 / (((xd - m.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3)) + f32(c.eps)).sqrt()
    return dict(x=x, gamma=d(F) if pas is EXACT else 1.0 + 0.2 * d(F), beta=d(F), dy=d(H, B, F, W), mean=m.float(), rstd=r.float())


def cl_reference(c, pas, inp, dtype, prec='f32'):
    t = dict((k, v.to(dtype)) for k, v in inp.items())
    H, B, F, W = c.shape
    pw = lambda k: t[k].unsqueeze(1) if k not in c.absent else torch.zeros(1, dtype=dtype)  # noqa: E731
    fb = f32(c.fb)
    if c.op == 'peep_fwd':
        y = t['y']
        yj, yi, yf, yo = (y[:, :, k * F:(k + 1) * F] for k in range(4))
        return dict(j=yj, ip=yi + pw('wci') * t['c'], fp=yf + pw('wcf') * t['c'], o=yo, _bit=('j', 'o'))
    if c.op == 'peep_bwd':
        out = dict(dy=torch.cat([t['dj'], t['di'], t['df'], t['do']], 2), dc=t['dc0'] + t['di'] * pw('wci') + t['df'] * pw('wcf'))
        if 'dwci' not in c.absent:
            out['dwci'] = (t['di'] * t['c']).sum(1)
        if 'dwcf' not in c.absent:
            out['dwcf'] = (t['df'] * t['c']).sum(1)
        return dict(out, _bit=('dy',))
    if c.op == 'cell_fwd':
        v = t['c'] * sig(t['f'] + fb) + sig(t['i']) * torch.tanh(t['j'])
        return dict(c_new=v, o_pre=t['o'] + pw('wco') * v)
    if c.op == 'cell_bwd':
        g = t['dcn0'] + t['dop'] * pw('wco')
        sf, si, tj = sig(t['f'] + fb), sig(t['i']), torch.tanh(t['j'])
        out = dict(dcn=g, dc=g * sf, df=g * t['c'] * sf * (1 - sf), di=g * tj * si * (1 - si), dj=g * si * (1 - tj * tj))
        if 'dwco' not in c.absent:
            out['dwco'] = (t['dop'] * t['cn']).sum(1)
        return dict(out, _int=('dwco',), _bit=('dcn',) if 'wco' in c.absent else ())
    if c.op == 'out_fwd':
        return dict(h=sig(t['o']) * torch.tanh(t['c']))
    if c.op == 'out_bwd':
        so, tc = sig(t['o']), torch.tanh(t['c'])
        return dict(do=t['dh'] * tc * so * (1 - so), dc=t['dh'] * so * (1 - tc * tc))
    # TF contrib layer_norm per sample b over (H, F, W); gamma / beta per feature
    x, dy = t['x'], t['dy']
    n = H * F * W
    bc = lambda v: v.view(1, -1, 1, 1)  # noqa: E731
    fc = lambda v: v.view(1, 1, -1, 1)  # noqa: E731
    m = x.sum(dim=(0, 2, 3)) / n
    r = 1.0 / (((x - bc(m)) ** 2).sum(dim=(0, 2, 3)) / n + f32(c.eps)).sqrt()
    y = (x - bc(m)) * bc(r) * fc(t['gamma']) + fc(t['beta'])
    xh = (x - bc(t['mean'])) * bc(t['rstd'])                      # (the backward takes mean / rstd as stored: fp32 values)
    g = dy * fc(t['gamma'])
    m1, m2 = g.sum(dim=(0, 2, 3)) / n, (g * xh).sum(dim=(0, 2, 3)) / n
    out = dict(y=y, mean=m, rstd=r, dx=bc(t['rstd']) * (g - bc(m1) - xh * bc(m2)), dgp=(dy * xh).sum(dim=(0, 3)), dbp=dy.sum(dim=(0, 3)))
    flat = n == 1 or c.special == 'const'       # x - mean is exactly zero: y = beta and the dgamma partials 0, bit for bit
    scale = {}
    if n == 1:      # dx = rstd (g - g) is identically zero; a fused multiply-add leaves the rounding of g, times rstd: the error is
        scale['dx'] = float((bc(t['rstd']) * g).abs().max())      # taken as a fraction of rstd |g|, the size of the terms that cancel
    return dict(out, _int=('dbp',), _bit=('y', 'mean', 'dgp') if flat and pas is REAL else (), _scale=scale)


def cl_run(Kmod, c, pas, inp, device, prec='f32'):
    H, B, F, W = c.shape
    kernel = cl_plan(c)['kernel']
    dev = lambda k: in_flat(inp[k], device) if k not in c.absent else None  # noqa: E731
    frames = {}

    def outw(name, kind='m', fill=None):
        if name in c.absent:
            return None
        shp = _cl_shape(kind, c.shape)
        frames[name] = FlatFrame(shp, device, nan(*shp) if fill is None else fill)
        return frames[name].win
    if c.op == 'peep_fwd':
        Kmod.convlstm_peephole_fwd(dev('y'), dev('c'), dev('wci'), dev('wcf'), outw('j'), outw('ip'), outw('fp'), outw('o'))
    elif c.op == 'peep_bwd':
        Kmod.convlstm_peephole_bwd(dev('dj'), dev('di'), dev('df'), dev('do'), dev('c'), dev('wci'), dev('wcf'), outw('dy', 'y4'),
                                   outw('dc', 'm', inp['dc0']), outw('dwci', 'p'), outw('dwcf', 'p'))
    elif c.op == 'cell_fwd':
        Kmod.convlstm_cell_fwd(dev('j'), dev('i'), dev('f'), dev('c'), dev('o'), dev('wco'), c.fb, outw('c_new'), outw('o_pre'))
    elif c.op == 'cell_bwd':
        dcn = outw('dcn', 'm', inp['dcn0'])
        Kmod.convlstm_cell_bwd(dev('j'), dev('i'), dev('f'), dev('c'), dev('cn'), dev('wco'), c.fb, dcn, dev('dop'), outw('dj'),
                               outw('di'), outw('df'), outw('dc'), outw('dwco', 'p'))
    elif c.op == 'out_fwd':
        Kmod.convlstm_out_fwd(dev('o'), dev('c'), outw('h'))
    elif c.op == 'out_bwd':
        Kmod.convlstm_out_bwd(dev('o'), dev('c'), dev('dh'), outw('do'), outw('dc'))
    else:
        for k, shp in (('y', (H, B, F, W)), ('mean', (B,)), ('rstd', (B,)), ('dx', (H, B, F, W)), ('dgp', (B, F)), ('dbp', (B, F))):
            frames[k] = FlatFrame(shp, device, nan(*shp))
        x, gamma = dev('x'), dev('gamma')
        Kmod.layer_norm_hbfw_fwd(x, gamma, dev('beta'), c.eps, frames['y'].win, frames['mean'].win, frames['rstd'].win)
        Kmod.layer_norm_hbfw_bwd(dev('dy'), x, gamma, dev('mean'), dev('rstd'), frames['dx'].win, frames['dgp'].win, frames['dbp'].win)
    return results(frames, kernel)


def cl_coverage(seen):
    for op in ('peep_fwd', 'peep_bwd', 'cell_fwd', 'cell_bwd', 'out_fwd', 'out_bwd'):
        q = [(c, pl) for _, c, pl in seen if c.op == op]
        _need((op, 'second grid-stride round'), (pl['rounds'] == 2 for c, pl in q))
        _need((op, 'H != B, both above 1'), (c.shape[0] != c.shape[1] and min(c.shape[:2]) > 1 for c, pl in q))
        if op.startswith('out'):
            continue
        for i, vals in enumerate(((1, 3), (1, 2), (1, 4, 5), (1, 16, 37))):
            for v in vals:
                _need((op, 'HBFW'[i], v), (c.shape[i] == v for c, pl in q))
    of = lambda op: [c for _, c, pl in seen if c.op == op]  # noqa: E731
    for op, names in (('peep_fwd', ('wci', 'wcf')), ('peep_bwd', ('wci', 'wcf'))):
        for n in names:
            _need((op, 'absent alone', n), (n in c.absent and len([a for a in c.absent if a in names]) == 1 for c in of(op)))
        _need((op, 'all peephole weights absent'), (all(n in c.absent for n in names) for c in of(op)))
    for n in ('dwci', 'dwcf'):
        _need(('peep_bwd gradient output absent', n), (n in c.absent and n.replace('d', '', 1) not in c.absent for c in of('peep_bwd')))
    _need('cell_fwd wco absent', ('wco' in c.absent for c in of('cell_fwd')))
    _need('cell_bwd dwco absent alone', (c.absent == ('dwco',) for c in of('cell_bwd')))
    _need('cell_bwd wco absent', ('wco' in c.absent for c in of('cell_bwd')))
    for op in ('cell_fwd', 'cell_bwd'):
        for fb in (0.0, 1.0):
            _need((op, 'forget_bias', fb), (c.fb == fb for c in of(op)))
    ln = [(c, pl) for _, c, pl in seen if c.op == 'ln']
    for n in (1, 96, 255, 256, 257, 3000):
        _need(('layer norm sample of', n), (pl['sample'] == n for c, pl in ln))
    _need('layer norm F 300', (c.shape[2] == 300 and pl['fiters'] == 2 for c, pl in ln))
    for eps in (1e-12, 1e-5):
        _need(('layer norm eps', eps), (c.eps == eps for c, pl in ln))
        _need(('layer norm constant sample, eps', eps), (c.eps == eps and c.special == 'const' for c, pl in ln))
    _need('layer norm mean 1000, spread 1', (c.special == 'mean1000' for c, pl in ln))
    _need('layer norm mean 1000, spread 1, mean not representable', (c.special == 'mean1000 plain' for c, pl in ln))


def _cl_passes(c):
    if c.op in ('peep_fwd', 'peep_bwd'):
        return (EXACT, REAL)
    if c.op in ('cell_bwd', 'ln'):
        return (EXACT, REAL)           # (the exact pass checks the weight-gradient sums / dbeta partials alone: '_int')
    return (REAL,)


FAMILIES['cl'] = Family(cl_cases, cl_plan, cl_inputs, cl_reference, cl_run, cl_coverage, _cl_passes)

ORDER = ('wn', 'cells', 'bce', 'elem', 'opt', 'tm', 'tr', 'rd', 'cl')
assert sorted(ORDER) == sorted(FAMILIES)

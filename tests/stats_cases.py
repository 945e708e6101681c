"""Shared pieces of the statistics launch fuzz (test_stats_fuzz.py on the GPU, test_stats_fuzz_host.py against the CPU models)
--  TEST INFRASTRUCTURE, no test functions, no GPU code imported at module level.

The six entry points a run is judged by, one family each:
  logit    ag_logit_summary  (logit_summary_kernel)                       csrc/pointwise.hip
  vec      ag_vec_stats      (vec_stats_kernel)                           csrc/pointwise.hip
  sqnorm   ag_sqnorm_rows    (sqnorm_rows_kernel, sqnorm_finish_kernel)   csrc/pointwise.hip
  commit   ag_summary_commit (summary_commit_kernel)                      csrc/pointwise.hip
  ltas     ag_ltas_power     (ltas_power_kernel, ltas_finish_kernel)      csrc/evalstats.hip
  score    ag_score_accum    (score_accum_kernel)                         csrc/evalstats.hip
Per family (FAMILIES[name]), the parts of a family of tests/pointwise_cases.py:
  cases()               [(label, Case)]: pinned, each at the smallest shape that reaches its branch.
  plan(c)               the branch or branches the call takes, restated from sizes, pitches and addresses alone; 'kernel' is
                        the name ag_last_kernel has to report.
  inputs(c, pas, seed)  CPU operands of one PASS: EXACT integers in [-3, 3] (every partial sum an integer below 2^53), REAL the
                        value classes of the case.
  reference(c, pas, inp) float64, restated from the contracts of include/audiogan_hip.h (tests/summary_model.py and
                        tests/eval_model.py are NOT called: they are the fp32 models the FLOOR is taken from).
  run(Kmod, c, pas, inp, device)
                        every output is a window in a sentinel frame, NaN-filled when the call writes and at a known start when
                        it accumulates; every input is a window in a frame of another filler, and what the contract says is
                        never read (padding, samples at or past a length, masked entries) holds NaN.
                        -> {output: dict(out, frame_ok, kernel)}
  check(tag, c, pas, pl, inp, ref, got, low, worst)
                        the bound rule of the family (below).
  coverage(seen)        one assertion per class the issue names.
sweep() walks a family: frames untouched, the kernel name, a second run with identical bits, then the family's rule:
  logit, vec   every operation of the kernel is a double and the result is rounded once: each word within ONE fp32 unit in
               the last place of fl32(float64 reference); counts, the fp32 quotient and, in the exact pass, the means: the bits.
  sqnorm       floor = error of summary_model.sqnorm_rows against float64 as a fraction of the value, not below 2^-24;
               bound = 16 x floor, never above the 1e-5 of tests/test_summary.py.
  commit       the bits, always.
  ltas         floor = error of eval_model.ltas_power per clip as a fraction of the clip's largest bin, not below 2^-24;
               bound = 16 x floor, never above eval_model.LTAS_BOUND; Parseval's sum as a second reference.
  score        words 0, 2, 3 exact; word 1 floor from eval_model.score_accum, 16 x, never above 1e-6; words 4 and 5 within
               n 2^-52 of sum |x| and of sum x^2 (absolute) plus one double rounding of the caller's word per call.
A margin above 16 and at most 64 would go into MARGINS with its measured ratio and its reason; none is needed
(profiles/stats_fuzz.txt)."""
import collections
import math
import struct

import numpy as np
import torch

from tests import eval_model as EM
from tests import summary_model as SM
from tests.conv_cases import (Frame, FlatFrame, StridedFrame, place, bound, margin_of, MARGIN, MARGIN_MAX, FLOOR_MIN,  # noqa: F401
                              EXACT, REAL, GUARD, cdiv)

NAN = float('nan')
COLS = 16                   # AG_SUMMARY_COLS
SCORE_WORDS = 6
LT_N, LT_HOP, LT_BINS, LT_CH = 256, 128, 129, 16
LIMIT = 1 << 22             # B T of ag_logit_summary and ag_score_accum
SQNORM_CEIL = 1e-5          # the rtol of tests/test_summary.py
SCORE_CEIL = 1e-6           # eval_model.check_scores, word 1

# (kernel, output) -> (a margin above 16 and at most 64, the measured ratio, the reason).  None is needed.
MARGINS = {}


class Case(dict):
    __getattr__ = dict.__getitem__


Family = collections.namedtuple('Family', 'cases plan inputs reference run check coverage passes floor')
FAMILIES = {}
_CACHE = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _need(what, it):
    assert any(it), ('never reached', what)


def _margin(kernel, output):
    m = MARGINS[(kernel, output)][0] if (kernel, output) in MARGINS else margin_of(kernel, output)
    assert MARGIN <= m <= MARGIN_MAX
    return m


def f32(v):
    """a Python number as the fp32 value the C ABI receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def same(out, want):
    """the bits, where every NaN stands for every other (0 / 0 has the sign the machine gives it)"""
    return bool(((bits(out) == bits(want)) | (torch.isnan(out) & torch.isnan(want))).all())


def ulps(out, ref):
    """|out - fl32(ref)| in units of the last place of fl32(ref)"""
    r32 = ref.float()
    gap = (torch.nextafter(r32.abs(), torch.tensor(float('inf'))) - r32.abs()).double()
    return (out.double() - r32.double()).abs() / gap


def last_kernel(Kmod, pl):
    return Kmod.lib.ag_last_kernel().decode() if hasattr(Kmod, 'lib') else pl['kernel']


def res(fr, kernel):
    return dict(out=fr.window(), frame_ok=fr.untouched(), kernel=kernel)


# ---- views ------------------------------------------------------------------------------------------------------------
#   'c'    a contiguous [B, T]                         'p'    rows at pitch T + 3, one float behind an aligned address
#   't'    the heads' transposed view of a [T, B] buffer (sxb = 1, sxt = B)
#   'col'  a [B, 1] column cut with a step from a [B, 5] buffer (buf[:, 2::5]): sxt = 5 at T == 1
def view2(kind, B, T):
    """(strides, offset in floats) of a [B, T] view"""
    assert kind != 'col' or T == 1
    return dict(c=((T, 1), 0), p=((T + 3, 1), 1), t=((1, B), 2), col=((5, 5), 2))[kind]


def in_view(x, kind, device):
    """an input [B, T] in view form `kind`; every float of the frame outside the view is NaN"""
    st, off = view2(kind, *x.shape)
    return StridedFrame(tuple(x.shape), st, off, device, x, sentinel=NAN).win


def in_rows(x, pitch, off, device):
    """an input [B, L] of unit column stride at row pitch `pitch`, `off` floats behind a 16-byte aligned address; the
    padding columns and the frame hold NaN"""
    w = StridedFrame(tuple(x.shape), (pitch, 1), off, device, x, sentinel=NAN).win
    assert torch.device(device).type == 'cpu' or w.data_ptr() % 16 == (4 * off) % 16
    return w


def in_ints(t, device, dtype=torch.int64):
    """a length table between guard words of -12345 (a negative length: a read past the table shows)"""
    return FlatFrame(tuple(t.shape), device, t, dtype=dtype).win if t is not None else None


NF_KINDS = ('none', 'mixed', 'neg', 'zero')


def nf_of(kind, B, T, gen):
    """nframes int64 [B]: 'mixed' holds a T + 4 (which clamps), a 0, a 1 and a T in its first four entries"""
    if kind == 'none':
        return None
    if kind == 'zero':
        return torch.zeros(B, dtype=torch.int64)
    v = torch.randint(0, T + 1, (B,), generator=gen)
    for i, n in enumerate((T + 4, 0, 1, T)[:B]):
        v[i] = n
    if kind == 'neg':
        v[B - 1] = -3
    return v


def nf_clamped(nf, B, T):
    return np.full(B, T, dtype=np.int64) if nf is None else np.clip(nf.numpy(), 0, T)


VALS = ('pin', 'big', 'zer')


def values(kind, pas, gen, *shape):
    """EXACT: integers in [-3, 3].  REAL: 'pin' 0.03 + 0.004 randn (the pinned step); 'big' 1000 + 1e-3 randn (fp32 spacing
    6e-5: the spread is resolvable, a one-pass fp32 variance is not); 'zer' 1.5 randn with an exact 0.0 and a -0.0"""
    if pas is EXACT:
        return torch.randint(-3, 4, shape, generator=gen).float()
    r = torch.randn(*shape, generator=gen, dtype=torch.float64)
    if kind == 'pin':
        return (0.03 + 0.004 * r).float()
    if kind == 'big':
        return (1000.0 + 1e-3 * r).float()
    x = (1.5 * r).float()
    flat = x.view(-1)
    flat[flat.numel() // 3] = 0.0
    flat[(2 * flat.numel()) // 3] = -0.0
    return x


# =====================================================================================================================
# 1. logit: ag_logit_summary
# =====================================================================================================================
LOGIT_WORDS = ('mean', 'std', 'hits', 'mask', 'ratio')
LOGIT_BT = ((1, 1), (1, 65), (65, 1), (3, 5), (7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (64, 128))


def logit_cases():
    out, k = [], 0

    def add(B, T, view, nf, val, pos):
        out.append(('%dx%d %s nf-%s %s pos%d' % (B, T, view, nf, val, pos), Case(B=B, T=T, view=view, nf=nf, val=val, pos=pos)))
    for B, T in LOGIT_BT:
        for view in ('c', 'p', 't') + (('col',) if T == 1 else ()):
            add(B, T, view, NF_KINDS[k % 4], VALS[k % 3], k % 2)
            k += 1
    add(3, 5, 'c', 'zero', 'pin', 1)            # every clip empty: words 2 and 3 exactly 0, word 4 the NaN of 0 / 0 in fp32
    add(7, 9, 't', 'mixed', 'big', 0)
    add(25, 41, 'p', 'neg', 'zer', 1)
    add(64, 128, 't', 'mixed', 'big', 1)
    add(2048, 2048, 'c', 'mixed', 'pin', 1)     # 2^22, the limit: 4096 trips of the stride loop
    return out


def logit_plan(c):
    st, _ = view2(c.view, c.B, c.T)
    return dict(kernel='logit_summary_kernel', tfast=int(st[1] == 1), trips=cdiv(c.B * c.T, 1024))


def logit_inputs(c, pas, seed):
    gen = _gen(seed)
    return dict(x=values(c.val, pas, gen, c.B, c.T), nf=nf_of(c.nf, c.B, c.T, gen))


def logit_reference(c, pas, inp):
    x = inp['x'].double().numpy()
    n = x.size
    mean = x.sum() / n
    std = math.sqrt(((x - mean) ** 2).sum() / n)                      # population, over ALL entries (masked ones count)
    nf = np.full(c.B, c.T, dtype=np.int64) if inp['nf'] is None else inp['nf'].numpy()
    mask = np.arange(c.T)[None, :] < nf[:, None]
    hit = ((x > 0) if c.pos else (x < 0)) & mask
    h, m = float(hit.sum()), float(mask.sum())
    ratio = float(torch.tensor(h, dtype=torch.float32) / torch.tensor(m, dtype=torch.float32))      # the fp32 division
    return dict(out=torch.tensor([mean, std, h, m, ratio], dtype=torch.float64))


def logit_run(Kmod, c, pas, inp, device):
    pl = logit_plan(c)
    fr = FlatFrame((5,), device, torch.full((5,), NAN))
    Kmod.logit_summary(in_view(inp['x'], c.view, device), in_ints(inp['nf'], device), c.pos, out=fr.win)
    return dict(out=res(fr, last_kernel(Kmod, pl)))


def words_check(tag, pas, names, ref, out, exact, worst, kernel):
    """logit / vec: `exact` words by their bits, the others within one fp32 unit in the last place"""
    for i, name in enumerate(names):
        t = (tag[0], tag[1], name)
        r, o = ref[i:i + 1], out[i:i + 1]
        if name in exact or float(r) == 0.0:
            assert same(o, r.float()), ('%s pass: word differs in its bits from fl32(float64 reference)' % pas['name'], t, float(o), float(r))
            continue
        assert bool(torch.isfinite(o).all()), ('NaN or infinity in the output', t, float(o))
        u = float(ulps(o, r))
        assert u <= 1.0, ('%s pass: more than one unit in the last place off' % pas['name'], t, float(o), float(r), u)
        if worst is not None:
            key = '%s:%s (units in the last place)' % (kernel, name)
            worst[key] = max(worst.get(key, 0.0), u)


def logit_check(tag, c, pas, pl, inp, ref, got, low, worst):
    exact = ('hits', 'mask', 'ratio') + (('mean',) if pas is EXACT else ())
    words_check(tag, pas, LOGIT_WORDS, ref['out'], got['out']['out'], exact, worst, pl['kernel'])


def logit_coverage(seen):
    for B, T in LOGIT_BT + ((2048, 2048),):
        _need(('logit shape', B, T), (c.B == B and c.T == T for _, c, pl in seen))
    for v in ('c', 'p', 't', 'col'):
        _need(('logit view', v), (c.view == v for _, c, pl in seen))
    for tf in (0, 1):
        _need(('logit index order tfast', tf), (pl['tfast'] == tf and c.B > 1 and c.T > 1 for _, c, pl in seen))
    _need('logit sxt != 1 at T == 1', (pl['tfast'] == 0 and c.T == 1 for _, c, pl in seen))
    for nf in NF_KINDS:
        _need(('logit nframes', nf), (c.nf == nf for _, c, pl in seen))
    _need('logit nframes with a 0, a 1, a T and a T + 4', (c.nf == 'mixed' and c.B >= 4 for _, c, pl in seen))
    _need('logit mixed nframes on the transposed view', (c.nf == 'mixed' and c.B >= 4 and c.view == 't' for _, c, pl in seen))
    for val in VALS:
        for pos in (0, 1):
            _need(('logit values', val, pos), (c.val == val and c.pos == pos for _, c, pl in seen))
    _need('logit 1000 + 1e-3 randn beyond one trip', (c.val == 'big' and pl['trips'] > 1 for _, c, pl in seen))
    for trips in (1, 2, 4096):
        _need(('logit trips', trips), (pl['trips'] == trips for _, c, pl in seen))


FAMILIES['logit'] = Family(logit_cases, logit_plan, logit_inputs, logit_reference, logit_run, logit_check, logit_coverage,
                           lambda c: (EXACT, REAL), False)


# =====================================================================================================================
# 2. vec: ag_vec_stats
# =====================================================================================================================
VEC_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097)
VEC_SIGNS = (1.0, -1.0, 0.5)


def vec_cases():
    out, k = [], 0
    for n in VEC_N:
        for _ in range(3 if n in (1, 257) else 2):
            c = Case(n=n, sign=VEC_SIGNS[k % 3], off=k % 2, val=VALS[(k // 2) % 3])
            out.append(('n%d sign%g off%d %s' % (n, c.sign, c.off, c.val), c))
            k += 1
    return out


def vec_plan(c):
    return dict(kernel='vec_stats_kernel', trips=cdiv(c.n, 256))


def vec_inputs(c, pas, seed):
    return dict(v=values(c.val, pas, _gen(seed), c.n))


def vec_reference(c, pas, inp):
    x = inp['v'].double().numpy()
    mean = x.sum() / c.n
    return dict(out=torch.tensor([c.sign * mean, math.sqrt(((x - mean) ** 2).sum() / c.n)], dtype=torch.float64))


def vec_run(Kmod, c, pas, inp, device):
    pl = vec_plan(c)
    v = StridedFrame((c.n,), (1,), c.off, device, inp['v'], sentinel=NAN).win
    fr = FlatFrame((2,), device, torch.full((2,), NAN))
    Kmod.vec_stats(v, c.sign, out=fr.win)
    return dict(out=res(fr, last_kernel(Kmod, pl)))


def vec_check(tag, c, pas, pl, inp, ref, got, low, worst):
    # (n == 1: the reference std is 0 and the word has to be +0 in its bits)
    words_check(tag, pas, ('mean', 'std'), ref['out'], got['out']['out'], ('mean',) if pas is EXACT else (), worst, pl['kernel'])


def vec_coverage(seen):
    for n in VEC_N:
        _need(('vec n', n), (c.n == n for _, c, pl in seen))
    for s in VEC_SIGNS:
        _need(('vec sign', s), (c.sign == s for _, c, pl in seen))
        _need(('vec sign beyond one trip', s), (c.sign == s and pl['trips'] > 1 for _, c, pl in seen))
    for off in (0, 1):
        _need(('vec base offset', off), (c.off == off for _, c, pl in seen))
    for val in VALS:
        _need(('vec values', val), (c.val == val for _, c, pl in seen))
    _need('vec 1000 + 1e-3 randn beyond one trip', (c.val == 'big' and pl['trips'] > 1 for _, c, pl in seen))
    for trips in (1, 2, 17):
        _need(('vec trips', trips), (pl['trips'] == trips for _, c, pl in seen))


FAMILIES['vec'] = Family(vec_cases, vec_plan, vec_inputs, vec_reference, vec_run, vec_check, vec_coverage,
                         lambda c: (EXACT, REAL), False)


# =====================================================================================================================
# 3. sqnorm: ag_sqnorm_rows (+ the mean ag_summary_commit takes of `part`)
# =====================================================================================================================
SQ_L = (1, 3, 4, 5, 1020, 1024, 1028, 4100)
SQ_COMMIT_COL = 3


def sqnorm_cases():
    out = []
    #    B   L     pitch - L  base  nframes  scale finish commit
    for B, L, dp, off, nf, scale, fin, com in (
            (1, 1, 0, 0, 'none', 1, 1, 1), (5, 3, 1, 1, 'mixed', 25, 1, 0), (5, 4, 0, 0, 'none', 4096, 1, 0),
            (5, 4, 1, 0, 'mixed', 1, 0, 0), (5, 4, 4, 2, 'none', 25, 1, 0), (2, 5, 0, 3, 'mixed', 1, 1, 1),
            (5, 1020, 1, 0, 'none', 1, 1, 0), (1, 1020, 0, 0, 'mixed', 25, 0, 0), (5, 1020, 4, 3, 'mixed', 4096, 1, 0),
            (5, 1024, 0, 0, 'mixed', 4096, 1, 0), (5, 1024, 1, 1, 'none', 1, 1, 0), (5, 1028, 4, 0, 'none', 1, 1, 0),
            (5, 1028, 1, 3, 'mixed', 25, 0, 0), (5, 4100, 1, 0, 'mixed', 25, 1, 0), (1, 4100, 0, 1, 'none', 1, 0, 0),
            (65, 4, 1, 0, 'mixed', 1, 1, 1), (65, 5, 4, 2, 'none', 4096, 1, 0), (65, 1024, 4, 0, 'mixed', 25, 1, 0),
            (65, 3, 0, 0, 'mixed', 1, 0, 0)):
        out.append(('B%d L%d pitch+%d base%d nf-%s scale%d fin%d commit%d' % (B, L, dp, off, nf, scale, fin, com),
                    Case(B=B, L=L, dp=dp, off=off, nf=nf, scale=scale, finish=fin, commit=com)))
    return out


def sqnorm_plan(c):
    """per row the path it takes: 'vec' (16-byte loads) iff the row's address is 16-byte aligned and L % 4 == 0"""
    ld = c.L + c.dp
    rows = ['vec' if (c.off + b * ld) % 4 == 0 and c.L % 4 == 0 else 'scalar' for b in range(c.B)]
    return dict(kernel='sqnorm_rows_kernel', rows=rows, ld=ld,
                trips=dict(vec=cdiv(c.L // 4, 256), scalar=cdiv(c.L, 256)))


def sqnorm_inputs(c, pas, seed):
    gen = _gen(seed)
    x = torch.randn(c.B, c.L, generator=gen) * torch.tensor([(1.0, 0.01, 30.0)[b % 3] for b in range(c.B)]).view(-1, 1)
    x = torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x)) * x.abs().clamp(1e-6, 1e3)     # magnitudes in [1e-6, 1e3]
    nf = None
    if c.nf == 'mixed':
        nf = torch.randint(1, c.L + 1, (c.B,), generator=gen)
        nf[c.B // 2] = 1
    return dict(x=x, nf=nf, scale=float(c.scale))


def sqnorm_reference(c, pas, inp):
    n = torch.full((c.B,), float(c.L), dtype=torch.float64) if inp['nf'] is None else inp['nf'].double()
    part = f32(inp['scale']) * (inp['x'].double() ** 2).sum(1) / n
    out = dict(part=part)
    if c.finish or c.commit:
        out['out'] = (part.sum() / c.B).view(1)
    if c.commit:
        out['commit'] = out['out']
    return out


def sqnorm_run(Kmod, c, pas, inp, device):
    pl = sqnorm_plan(c)
    gx = in_rows(inp['x'], pl['ld'], c.off, device)
    nf = in_ints(inp['nf'], device)
    part = FlatFrame((c.B,), device, torch.full((c.B,), NAN))
    got = {}
    if c.commit:
        # the form the training loop uses: no finishing launch, `part` handed to ag_summary_commit, which takes the same mean
        Kmod.sqnorm_rows(gx, nf, inp['scale'], part=part.win, finish=False)
        kernel = last_kernel(Kmod, pl)
        ring = FlatFrame((1, COLS), device, torch.full((1, COLS), 7777, dtype=torch.int32), dtype=torch.int32)
        cur = FlatFrame((2,), device, torch.tensor([0, 7], dtype=torch.int32), dtype=torch.int32)
        Kmod.summary_commit(ring.win, cur.win, [None] * COLS, part=part.win, part_col=SQ_COMMIT_COL)
        got['commit'] = dict(out=ring.window()[0, SQ_COMMIT_COL:SQ_COMMIT_COL + 1].view(torch.float32).clone(),
                             frame_ok=ring.untouched() and cur.untouched(), kernel=kernel)
        first = part.window()
    fo = None
    if c.finish or c.commit:
        fo = FlatFrame((1,), device, torch.full((1,), NAN))
    Kmod.sqnorm_rows(gx, nf, inp['scale'], part=part.win, out=fo.win if fo is not None else None, finish=fo is not None)
    kernel = last_kernel(Kmod, pl)
    got['part'] = res(part, kernel)
    if fo is not None:
        got['out'] = res(fo, kernel)
    if c.commit:
        assert same(first, got['part']['out']), ('sqnorm: part depends on the finishing launch', c)
    return got


def rel_check(tag, pas, ref, got, low, kernel, output, ceil, worst):
    """|out - ref| / |ref| per element under 16 x the model's (not below 2^-24), never above `ceil`"""
    t = (tag[0], tag[1], output)
    out = got['out'].reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), ('NaN or infinity in the output (an element not written, or padding read)', t)
    assert bool((ref != 0).all()), ('real pass: a reference value is zero, the case checks nothing', t)
    floor = float(((low.reshape(ref.shape).double() - ref).abs() / ref.abs()).max())
    err = float(((out.double() - ref).abs() / ref.abs()).max())
    b = min(bound(_margin(kernel, output), floor), ceil)
    assert err <= b, ('real pass: out of bound', t, err, floor, b)
    if worst is not None:
        key = '%s:%s' % (kernel, output)
        worst[key] = max(worst.get(key, 0.0), err / max(floor, FLOOR_MIN))


def sqnorm_check(tag, c, pas, pl, inp, ref, got, low, worst):
    for k in sorted(got):
        rel_check(tag, pas, ref[k], got[k], low[k], pl['kernel'], k, SQNORM_CEIL, worst)
    if c.commit:
        assert same(got['commit']['out'], got['out']['out']), \
            ("the ring word of ag_summary_commit has not the bits of ag_sqnorm_rows' out[0]", (tag[0], tag[1], 'commit'))


def sqnorm_coverage(seen):
    S = [(c, pl) for _, c, pl in seen]
    for L in SQ_L:
        _need(('sqnorm L', L), (c.L == L for c, pl in S))
    for dp in (0, 1, 4):
        _need(('sqnorm pitch L +', dp), (c.dp == dp and c.B > 1 for c, pl in S))
    for off in range(4):
        _need(('sqnorm base offset', off), (c.off == off for c, pl in S))
    for B in (1, 5, 65):
        _need(('sqnorm B', B), (c.B == B for c, pl in S))
    _need('sqnorm both paths in one launch (L % 4 == 0, odd pitch)',
          (c.L % 4 == 0 and c.dp % 2 and set(pl['rows']) == {'vec', 'scalar'} for c, pl in S))
    _need('sqnorm both paths in one launch, more than one trip', (set(pl['rows']) == {'vec', 'scalar'} and pl['trips']['vec'] > 1 for c, pl in S))
    _need('sqnorm all scalar: L % 4 != 0', (c.L % 4 and set(pl['rows']) == {'scalar'} and c.B > 1 for c, pl in S))
    _need('sqnorm all scalar: L % 4 == 0 behind a misaligned base', (c.L % 4 == 0 and set(pl['rows']) == {'scalar'} for c, pl in S))
    _need('sqnorm all 16-byte', (set(pl['rows']) == {'vec'} and c.B > 1 for c, pl in S))
    _need('sqnorm 16-byte path, L < 1024', (c.L < 1024 and c.L > 4 and 'vec' in pl['rows'] for c, pl in S))
    _need('sqnorm 16-byte path, two trips', ('vec' in pl['rows'] and pl['trips']['vec'] == 2 for c, pl in S))
    _need('sqnorm scalar path, 17 trips', ('scalar' in pl['rows'] and pl['trips']['scalar'] == 17 for c, pl in S))
    for nf in ('none', 'mixed'):
        _need(('sqnorm nframes', nf), (c.nf == nf for c, pl in S))
    for sc in (1, 25, 4096):
        _need(('sqnorm scale', sc), (c.scale == sc for c, pl in S))
    for fin in (0, 1):
        _need(('sqnorm finish', fin), (c.finish == fin and not c.commit for c, pl in S))
    for B in (1, 2, 65):
        _need(('sqnorm part handed to summary_commit, B', B), (c.commit and c.B == B for c, pl in S))


FAMILIES['sqnorm'] = Family(sqnorm_cases, sqnorm_plan, sqnorm_inputs, sqnorm_reference, sqnorm_run, sqnorm_check,
                            sqnorm_coverage, lambda c: (REAL,), True)


# =====================================================================================================================
# 4. commit: ag_summary_commit
# =====================================================================================================================
RING_FILL, SRC_FILL = 7777, 0x55555555
NAN_PAYLOAD, NEG_ZERO, SUBNORMAL, INT_MIN = 0x7FC12345, 0x80000000, 0x00000001, 0x80000000


def _s32(u):
    return struct.unpack('<i', struct.pack('<I', u & 0xFFFFFFFF))[0]


def _fbits(v):
    return struct.unpack('<I', struct.pack('<f', v))[0]


def commit_cases():
    out = []
    #    capacity  cursor row  sequence number  columns  part_col  npart  calls
    for cap, row, seq, cols, pc, npart, calls in (
            (1, 0, 0, 'imm', -1, 0, 1), (1, 0, 5, 'src16', -1, 0, 3), (2, 1, 2 ** 31 - 2, 'src16', -1, 0, 1),
            (2, 0, 11, 'mix', 0, 1, 5), (3, 2, 100, 'mix', 0, 3, 2), (3, 0, 1, 'imm', 1, 3, 1), (3, 1, 9, 'mix', 15, 65, 5),
            (2, 0, 3, 'src16', 15, 4096, 1), (3, 2, 40, 'src16', 1, 65, 4),
            (3, -1, 6, 'src16', -1, 0, 1), (3, 3, 6, 'imm', 0, 3, 1), (3, 5, 6, 'mix', -1, 0, 2), (1, 1, 6, 'imm', -1, 0, 1)):
        out.append(('cap%d row%d seq%d %s part_col%d npart%d calls%d' % (cap, row, seq, cols, pc, npart, calls),
                    Case(cap=cap, row=row, seq=seq, cols=cols, pc=pc, npart=npart, calls=calls)))
    return out


def commit_plan(c):
    refused = int(c.row < 0 or c.row >= c.cap)
    return dict(kernel='summary_commit_kernel', refused=refused, wraps=int(not refused and c.row + c.calls >= c.cap))


def commit_inputs(c, pas, seed):
    """cols: 16 of ('src', 'f' | 'i', the 32-bit word) / ('imm', a Python float, int or None)"""
    gen = _gen(seed)
    rnd = [int(v) for v in torch.randint(0, 2 ** 32, (COLS,), generator=gen)]
    special = {0: ('f', NAN_PAYLOAD), 1: ('i', 123), 2: ('f', NEG_ZERO), 3: ('f', SUBNORMAL), 4: ('i', INT_MIN)}
    src = [('src',) + special.get(i, ('fi'[i % 2], rnd[i] if i % 2 else _fbits(float(i) + 0.25))) for i in range(COLS)]
    imm = [('imm', v) for v in (1.5, 77, 2 ** 31 + 5, 2 ** 32 - 1, -0.0, None, -7, 0, 2.0 ** -140, 3, None, -2 ** 31, 1e30, 12, 0.1, 2 ** 31)]
    cols = dict(src16=src, imm=imm, mix=[src[i] if i % 2 == 0 else imm[i] for i in range(COLS)])[c.cols]
    if c.cols == 'mix':
        cols[1] = src[1]          # a src column at column 1 next to immediates: the sequence number wins
    part = None
    if c.npart:
        part = torch.randint(-3, 4, (c.npart,), generator=gen).float() if pas is EXACT else torch.randn(c.npart, generator=gen)
    return dict(cols=cols, part=part)


def commit_reference(c, pas, inp):
    ring = np.full((c.cap, COLS), RING_FILL, dtype=np.int64)
    row, seq = c.row, c.seq
    pm = None
    if inp['part'] is not None:
        s = 0.0
        for v in inp['part'].tolist():          # b ascending, in double
            s += v
        pm = _fbits(s / c.npart)
    for _ in range(c.calls):
        if row < 0 or row >= c.cap:
            continue                            # a cursor somebody overwrote: nothing is written, nothing advances
        for i, col in enumerate(inp['cols']):
            if i == 1:
                w = seq
            elif pm is not None and i == c.pc:
                w = pm
            elif col[0] == 'src':
                w = col[2]
            elif col[1] is None:
                w = 0
            else:
                w = _fbits(col[1]) if isinstance(col[1], float) else col[1]
            ring[row, i] = _s32(w)
        row, seq = (row + 1) % c.cap, seq + 1
    return dict(ring=torch.from_numpy(ring).to(torch.int32), cursor=torch.tensor([row, seq], dtype=torch.int32))


def commit_run(Kmod, c, pas, inp, device):
    pl = commit_plan(c)
    # the ring is a window with GUARD / 16 = 4 guard rows on either side inside ONE allocation: a launch without the cursor
    # check writes into the frame, not outside the allocation
    assert GUARD >= 4 * COLS
    ring = FlatFrame((c.cap, COLS), device, torch.full((c.cap, COLS), RING_FILL, dtype=torch.int32), dtype=torch.int32)
    cur = FlatFrame((2,), device, torch.tensor([c.row, c.seq], dtype=torch.int32), dtype=torch.int32)
    words = torch.full((3 * COLS,), _s32(SRC_FILL), dtype=torch.int32)
    for i, col in enumerate(inp['cols']):
        if col[0] == 'src':
            words[3 * i + 1] = _s32(col[2])
    words = words.to(device)
    cols = []
    for i, col in enumerate(inp['cols']):
        if col[0] == 'src':
            w = words[3 * i + 1:3 * i + 2]
            cols.append(w.view(torch.float32) if col[1] == 'f' else w)
        else:
            cols.append(col[1])
    part = StridedFrame((c.npart,), (1,), 1, device, inp['part'], sentinel=NAN).win if c.npart else None
    for _ in range(c.calls):
        Kmod.summary_commit(ring.win, cur.win, cols, part=part, part_col=c.pc)
    kernel = last_kernel(Kmod, pl)
    return dict(ring=res(ring, kernel), cursor=res(cur, kernel))


def commit_check(tag, c, pas, pl, inp, ref, got, low, worst):
    for k in ('ring', 'cursor'):
        assert torch.equal(got[k]['out'].reshape(ref[k].shape), ref[k]), \
            ('ring row, cursor or sequence number differs in its bits', (tag[0], tag[1], k), got[k]['out'], ref[k])


def commit_coverage(seen):
    S = [(c, pl) for _, c, pl in seen]
    for cap in (1, 2, 3):
        _need(('commit capacity', cap), (c.cap == cap and not pl['refused'] for c, pl in S))
        _need(('commit cursor starts at capacity - 1', cap), (c.cap == cap and c.row == cap - 1 for c, pl in S))
    _need('commit sequence number 2^31 - 2', (c.seq == 2 ** 31 - 2 for c, pl in S))
    for cols in ('src16', 'imm', 'mix'):
        _need(('commit columns', cols), (c.cols == cols and not pl['refused'] for c, pl in S))
    for pc in (0, 1, 15):
        _need(('commit part_col', pc), (c.pc == pc and c.npart and not pl['refused'] for c, pl in S))
    _need('commit part over a src column', (c.pc == 15 and c.cols == 'src16' and c.npart for c, pl in S))
    for npart in (1, 3, 65, 4096):
        _need(('commit npart', npart), (c.npart == npart and not pl['refused'] for c, pl in S))
    for row in (-1, 0, 2):
        _need(('commit refusal, cursor row capacity +', row), (pl['refused'] and c.row == (c.cap + row if row >= 0 else -1) and c.cap == 3
                                                               for c, pl in S))
    _need('commit wraps more than once', (c.calls > c.cap and not pl['refused'] for c, pl in S))


FAMILIES['commit'] = Family(commit_cases, commit_plan, commit_inputs, commit_reference, commit_run, commit_check,
                            commit_coverage, lambda c: (EXACT, REAL), False)


# =====================================================================================================================
# 5. ltas: ag_ltas_power
# =====================================================================================================================
# frames per L: 1 1 1 1 1 1 2 3 | 16 (the largest S == 1) | 17 (S == 2, ONE frame in the second chunk) 18 | 33 (S == 3).
# The issue's list gives 2304 as "16 frames, the largest S == 1" and 2432 as 17; by (L - 256) / 128 + 1 they have 17 and 18,
# so L = 2176 (16 frames) is added here for the class the issue describes, and 2304 is the one-frame second chunk.
LT_L = (1, 100, 255, 256, 257, 383, 384, 512, 2176, 2304, 2432, 4352)
LT_KINDS = ('randn', 'walk', 'sine', 'dc', 'nyq', 'tiny', 'big')
LT_EDGE = (0, -5, 521, 512, 300, 255, 256, 100, 384, 383)
LT_SHORT = (4352, 2304, 2303, 100, 2176)


def lt_frames(n):
    return (n - LT_N) // LT_HOP + 1 if n >= LT_N else 1


def ltas_cases():
    out, k = [], 0

    def add(L, lens, dp, off, kind, B=2):
        name = 'full' if lens is None else ('edge' if lens == LT_EDGE else ('short' if lens == LT_SHORT else 'given'))
        out.append(('L%d %s pitch+%d base%d %s' % (L, name, dp, off, kind),
                    Case(L=L, lens=lens, B=B if lens is None else len(lens), dp=dp, off=off, kind=kind)))
    for L in LT_L:
        add(L, None, (0, 7, 7, 0)[k % 4], (0, 1, 0, 1)[k % 4], LT_KINDS[k % 7])
        k += 1
    add(383, (383, 383), 7, 1, 'nyq')
    add(512, None, 7, 0, 'dc')
    add(2304, None, 0, 1, 'tiny')
    add(2432, (2432, 2304, 2176), 7, 1, 'big')
    add(512, LT_EDGE, 7, 1, 'randn')
    add(512, LT_EDGE, 0, 0, 'nyq')
    add(512, LT_EDGE, 7, 0, 'sine')
    add(4352, LT_SHORT, 7, 1, 'randn')
    add(4352, LT_SHORT, 0, 0, 'walk')
    add(4352, None, 7, 0, 'nyq', B=1)
    return out


def _lt_n(c):
    return [c.L] * c.B if c.lens is None else [max(0, min(int(n), c.L)) for n in c.lens]


def ltas_plan(c):
    S = cdiv(lt_frames(c.L), LT_CH)
    nf = [lt_frames(n) for n in _lt_n(c)]
    nc = [cdiv(f, LT_CH) for f in nf]
    return dict(kernel='ltas_power_kernel', S=S, nf=nf, nc=nc, ws=c.B * S * LT_BINS if S > 1 else 0,
                dead_odd=int(any(f % 2 for f in nf)), idle=int(any(q < S for q in nc)))


def ltas_inputs(c, pas, seed):
    rs = np.random.RandomState(seed)
    B, L = c.B, c.L
    t = np.arange(L, dtype=np.float64)
    if c.kind in ('randn', 'tiny', 'big'):
        x = rs.randn(B, L) * dict(randn=0.3, tiny=1e-6, big=1e3)[c.kind]
    elif c.kind == 'walk':
        x = np.cumsum(rs.randn(B, L) * 0.05, axis=1)
    elif c.kind == 'sine':      # bin-centred: an integer number of periods per frame
        x = 0.5 * np.sin(2.0 * np.pi * rs.randint(3, 120, size=(B, 1)) * t[None, :] / LT_N + rs.rand(B, 1)) + 1e-3 * rs.randn(B, L)
    elif c.kind == 'dc':
        x = np.full((B, L), 0.75)
    else:                       # 'nyq': the energy in the bins the k == 0 lane computes
        x = np.tile(0.5 * (-1.0) ** t, (B, 1))
    x = x.astype(np.float32)
    x2 = x.copy()               # the samples inside the clip but past its last whole frame replaced
    for b, n in enumerate(_lt_n(c)):
        cov = LT_N + LT_HOP * (lt_frames(n) - 1)
        if n >= LT_N and cov < n:
            x2[b, cov:n] = (7.0 + rs.randn(n - cov)).astype(np.float32)
        x[b, n:] = np.nan       # never read
        x2[b, n:] = np.nan
    return dict(x=torch.from_numpy(x), x2=torch.from_numpy(x2),
                lens=torch.tensor(c.lens, dtype=torch.int64) if c.lens is not None else None)


_HANN = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(LT_N, dtype=np.float64) / LT_N)
_PARSEVAL_W = np.array([1.0] + [2.0] * (LT_BINS - 2) + [1.0])


def ltas_reference(c, pas, inp):
    """P [B, 129] and, independent of any FFT, the mean over frames of sum_i (w_i x_i)^2 (Parseval)"""
    x = inp['x'].double().numpy()
    P, E = np.zeros((c.B, LT_BINS)), np.zeros(c.B)
    for b, n in enumerate(_lt_n(c)):
        nf = lt_frames(n)
        f = np.zeros((nf, LT_N))
        if n >= LT_N:
            for j in range(nf):
                f[j] = x[b, j * LT_HOP:j * LT_HOP + LT_N]
        else:
            f[0, :n] = x[b, :n]
        f = f * _HANN
        P[b] = (np.abs(np.fft.rfft(f, axis=1)) ** 2).mean(0)
        E[b] = (f * f).sum(1).mean()
    assert np.isfinite(P).all()
    return dict(out=torch.from_numpy(P), nframes=torch.tensor([lt_frames(n) for n in _lt_n(c)], dtype=torch.int32), energy=E)


def gpu_ltas_raw(K):
    """the C entry with a workspace of the test's own (sized by the plan, bound with ag_bind_workspace)"""
    def raw(x, lens, out, nframes, slab):
        B, L = x.shape
        ld = x.stride(0) if B > 1 else max(x.stride(0), L)
        assert K.lib.ag_bind_workspace(K._p(slab), slab.numel()) == 0
        rc = K.lib.ag_ltas_power(K._p(x), ld, K._p(lens), K._p(out), K._p(nframes), B, L, K._stream())
        assert rc == 0, K.lib.ag_last_error()
    return raw


def ltas_run(Kmod, c, pas, inp, device):
    pl = ltas_plan(c)
    if hasattr(Kmod, 'lib'):
        assert int(Kmod.lib.ag_ltas_ws_numel(c.B, c.L)) == pl['ws'], ('ag_ltas_ws_numel differs from the plan', c)
    lens = in_ints(inp['lens'], device)
    got = {}

    def once(x, raw):
        xw = in_rows(x, c.L + c.dp, c.off, device)
        out = FlatFrame((c.B, LT_BINS), device, torch.full((c.B, LT_BINS), NAN))
        nfr = FlatFrame((c.B,), device, torch.full((c.B,), -1, dtype=torch.int32), dtype=torch.int32)
        ws = None
        if raw:
            ws = FlatFrame((pl['ws'],), device, torch.full((pl['ws'],), NAN))
            (gpu_ltas_raw(Kmod) if hasattr(Kmod, 'lib') else Kmod.ltas_raw)(xw, lens, out.win, nfr.win, ws.win.view(c.B, pl['S'], LT_BINS))
        else:
            Kmod.ltas_power(xw, lens, out=out.win, nframes=nfr.win)
        return out, nfr, ws, last_kernel(Kmod, pl)
    out, nfr, ws, kernel = once(inp['x'], pl['S'] > 1)
    got['out'], got['nframes'] = res(out, kernel), res(nfr, kernel)
    if ws is not None:
        got['slab'] = res(ws, kernel)
        wrapped = once(inp['x'], False)[0]          # the wrapper binds a slab of the allocator's: the same bits
        got['wrapped'] = res(wrapped, kernel)
    got['tail'] = res(once(inp['x2'], pl['S'] > 1)[0], kernel)
    return got


def ltas_check(tag, c, pas, pl, inp, ref, got, low, worst):
    t = (tag[0], tag[1], 'out')
    out, P = got['out']['out'].double().numpy(), ref['out'].numpy()
    assert torch.equal(got['nframes']['out'], ref['nframes']), ('frame counts differ', (tag[0], tag[1], 'nframes'))
    assert np.isfinite(out).all(), ('NaN or infinity in the output (a sample at or past a length read, a chunk the clip does not have added, '
                                    'or a bin not written)', t)
    if 'slab' in got:
        slab = got['slab']['out'].view(c.B, pl['S'], LT_BINS)
        for b in range(c.B):
            assert bool(torch.isnan(slab[b, pl['nc'][b]:]).all()), ('a slab row of a chunk the clip does not have was written', (tag[0], tag[1], 'slab'), b)
            assert bool(torch.isfinite(slab[b, :pl['nc'][b]]).all()), ('a slab row the finishing launch reads was not written', (tag[0], tag[1], 'slab'), b)
        assert same(got['wrapped']['out'], got['out']['out']), ('the bits depend on whose workspace is bound', t)
    assert same(got['tail']['out'], got['out']['out']), ('samples past the last whole frame change the bits', (tag[0], tag[1], 'tail'))
    model = low['out'].double().numpy()
    for b in range(c.B):
        top = P[b].max()
        if top == 0.0:          # an empty clip: one frame of zeros, power exactly +0
            assert not got['out']['out'][b].view(torch.int32).any(), ('an empty clip has not power exactly +0', t, b)
            continue
        floor = np.abs(model[b] - P[b]).max() / top
        err = np.abs(out[b] - P[b]).max() / top
        bd = min(bound(_margin(pl['kernel'], 'out'), floor), EM.LTAS_BOUND)
        assert err <= bd, ('real pass: out of bound', t, b, err, floor, bd)
        # Parseval: sum_k w_k P[k] / 256 = mean over frames of sum_i (w_i x_i)^2, float64 and no FFT; 129 x the power bound
        assert abs((_PARSEVAL_W * P[b]).sum() / LT_N - ref['energy'][b]) <= 1e-12 * ref['energy'][b], ('the float64 reference misses Parseval', t, b)
        assert abs((_PARSEVAL_W * out[b]).sum() / LT_N - ref['energy'][b]) <= LT_BINS * bd * top, ('Parseval', t, b)
        if worst is not None:
            key = '%s:out (%s)' % (pl['kernel'], c.kind)
            worst[key] = max(worst.get(key, 0.0), err / max(floor, FLOOR_MIN))


def ltas_coverage(seen):
    S = [(c, pl) for _, c, pl in seen]
    for L in LT_L:
        _need(('ltas L', L), (c.L == L and c.lens is None for c, pl in S))
    for kind in LT_KINDS:
        _need(('ltas kind', kind), (c.kind == kind for c, pl in S))
        _need(('ltas kind over more than one chunk', kind), (c.kind == kind and pl['S'] > 1 for c, pl in S))
    for dp in (0, 7):
        for off in (0, 1):
            _need(('ltas pitch L +, base', dp, off), (c.dp == dp and c.off == off for c, pl in S))
    _need('ltas lens 0, negative, above L', (c.lens is not None and 0 in c.lens and min(c.lens) < 0 and max(c.lens) > c.L for c, pl in S))
    _need('ltas a zero-padded frame', (any(n < LT_N for n in _lt_n(c)) for c, pl in S))
    _need('ltas a dead odd half', (pl['dead_odd'] and max(pl['nf']) > 1 for c, pl in S))
    _need('ltas the largest S == 1', (pl['S'] == 1 and max(pl['nf']) == LT_CH for c, pl in S))
    _need('ltas S == 2 with one frame in the second chunk', (pl['S'] == 2 and LT_CH + 1 in pl['nf'] for c, pl in S))
    _need('ltas S == 3', (pl['S'] == 3 and max(pl['nc']) == 3 for c, pl in S))
    _need('ltas later chunks empty: workgroups return, the finishing launch reads nc chunks', (pl['S'] == 3 and {1, 2, 3} <= set(pl['nc']) for c, pl in S))
    _need('ltas a tail past the last whole frame', (any(n >= LT_N and (n - LT_N) % LT_HOP for n in _lt_n(c)) for c, pl in S))
    _need('ltas the Nyquist kind on one zero-padded and on 33 frames', (c.kind == 'nyq' and pl['S'] == 3 for c, pl in S))


FAMILIES['ltas'] = Family(ltas_cases, ltas_plan, ltas_inputs, ltas_reference, ltas_run, ltas_check, ltas_coverage,
                          lambda c: (REAL,), True)


# =====================================================================================================================
# 6. score: ag_score_accum
# =====================================================================================================================
SCORE_NAMES = ('clips', 'loss', 'frames', 'hits', 'sum', 'sumsq')
SCORE_B, SCORE_T = (1, 15, 16, 17, 33), (1, 63, 64, 65, 129)
BIG_START = 1e6
EXTREMES = (0.0, -0.0, 30.0, -30.0, 87.0, -87.0, 88.8, -88.8, 104.0, -104.0)     # around the under- and overflow of expf


def score_cases():
    out, k = [], 0
    for B in SCORE_B:
        for T in SCORE_T:
            views = ('c', 'p', 't') + (('col',) if T == 1 else ())
            c = Case(B=B, T=T, view=views[k % len(views)], nf=NF_KINDS[k % 4], start=('zero', 'big')[(k // 2) % 2],
                     calls=10 if (B, T) in ((17, 65), (1, 1)) else 1, val='ext' if T >= 63 and k % 3 == 0 else 'randn',
                     target=(0.9, 0.0, 0.5)[k % 3], pos=k % 2)
            out.append(('%dx%d %s nf-%s start-%s calls%d %s tg%g pos%d' % (B, T, c.view, c.nf, c.start, c.calls, c.val, c.target, c.pos), c))
            k += 1
    out.append(('33x129 t nf-mixed start-big calls1 ext tg0.9 pos1',
                Case(B=33, T=129, view='t', nf='mixed', start='big', calls=1, val='ext', target=0.9, pos=1)))
    out.append(('17x1 col nf-mixed start-big calls1 randn tg0.9 pos0',
                Case(B=17, T=1, view='col', nf='mixed', start='big', calls=1, val='randn', target=0.9, pos=0)))
    out.append(('16x64 c nf-zero start-big calls1 randn tg0.5 pos1',
                Case(B=16, T=64, view='c', nf='zero', start='big', calls=1, val='randn', target=0.5, pos=1)))
    return out


def score_plan(c):
    st, _ = view2(c.view, c.B, c.T)
    return dict(kernel='score_accum_kernel', rows_per_wave=cdiv(c.B, 16), lane_trips=cdiv(c.T, 64), tfast=int(st[1] == 1))


def score_inputs(c, pas, seed):
    gen = _gen(seed)
    x = values('zer', pas, gen, c.B, c.T)          # 1.5 randn with an exact 0.0 and a -0.0: neither sign
    nf = nf_of(c.nf, c.B, c.T, gen)
    if c.val == 'ext' and pas is REAL:
        x[0, :len(EXTREMES)] = torch.tensor(EXTREMES)          # row 0 is whole in every nframes kind but 'zero'
    for b, n in enumerate(nf_clamped(nf, c.B, c.T)):
        x[b, int(n):] = NAN                                     # masked entries are never read
    start = torch.zeros(6, dtype=torch.float64) if c.start == 'zero' else torch.full((6,), BIG_START, dtype=torch.float64)
    return dict(x=x, nf=nf, start=start)


def score_reference(c, pas, inp):
    x = inp['x'].double().numpy()
    tg = f32(c.target)
    a, sabs, ntot = np.zeros(6), 0.0, 0
    for b, n in enumerate(nf_clamped(inp['nf'], c.B, c.T)):
        n = int(n)
        if n < 1:
            continue                                            # skipped, and not counted in word 0
        v = x[b, :n]
        m = np.maximum(-v, 0.0)
        per = v - v * tg + m + np.log(np.exp(-m) + np.exp(-v - m))
        a += [1.0, per.sum() / n, n, ((v > 0) if c.pos else (v < 0)).sum(), v.sum(), (v * v).sum()]
        sabs += np.abs(v).sum()
        ntot += n
    assert np.isfinite(a).all()
    acc = inp['start'].clone()
    for _ in range(c.calls):
        acc += torch.from_numpy(a)
    return dict(acc=acc, add=a, sabs=sabs, n=ntot)


def score_run(Kmod, c, pas, inp, device):
    pl = score_plan(c)
    acc = FlatFrame((6,), device, inp['start'], dtype=torch.float64)
    xw, nf = in_view(inp['x'], c.view, device), in_ints(inp['nf'], device)
    for _ in range(c.calls):
        Kmod.score_accum(xw, nf, c.target, c.pos, acc.win)
    return dict(acc=res(acc, last_kernel(Kmod, pl)))


def score_check(tag, c, pas, pl, inp, ref, got, low, worst):
    out, start, add = got['acc']['out'].double(), inp['start'], ref['add']
    assert bool(torch.isfinite(out).all()), ('NaN or infinity in the output (a masked entry read)', (tag[0], tag[1], 'acc'))
    for q, name in enumerate(SCORE_NAMES):
        t = (tag[0], tag[1], name)
        d, want = float(out[q] - start[q]), c.calls * float(add[q])          # (the difference of two doubles this close is exact)
        if q in (0, 2, 3) or (pas is EXACT and q != 1):
            assert float(out[q]) == float(ref['acc'][q]), ('%s pass: word differs from the float64 reference' % pas['name'], t, float(out[q]), float(ref['acc'][q]))
        elif q == 1:
            if pas is EXACT:
                continue                        # (transcendental: the real pass checks it)
            if want == 0.0:
                assert d == 0.0, ('real pass: out of bound', t, d)
                continue
            dl = float(low['acc'].double()[q] - start[q])
            floor, err = abs(dl - want) / abs(want), abs(d - want) / abs(want)
            b = min(bound(_margin(pl['kernel'], name), floor), SCORE_CEIL)
            assert err <= b, ('real pass: out of bound', t, err, floor, b)
            if worst is not None:
                key = '%s:%s' % (pl['kernel'], name)
                worst[key] = max(worst.get(key, 0.0), err / max(floor, FLOOR_MIN))
        else:
            # n 2^-52 of sum |x| (of sum x^2) for the double sums, whatever their order, and one rounding of the caller's
            # double per call; an fp32 temporary anywhere is orders of magnitude outside
            mag = ref['sabs'] if q == 4 else float(add[5])
            tol = c.calls * (ref['n'] * 2.0 ** -52 * mag + 2.0 ** -52 * max(abs(float(start[q])), abs(float(out[q]))))
            assert abs(d - want) <= tol, ('real pass: out of bound', t, d, want, tol)


def score_coverage(seen):
    S = [(c, pl) for _, c, pl in seen]
    for B in SCORE_B:
        _need(('score B', B), (c.B == B for c, pl in S))
    for T in SCORE_T:
        _need(('score T', T), (c.T == T for c, pl in S))
    for r in (1, 2, 3):
        _need(('score rows per wave', r), (pl['rows_per_wave'] == r for c, pl in S))
        _need(('score lane trips', r), (pl['lane_trips'] == r for c, pl in S))
    _need('score second row of a wave and second trip of the lanes in one call', (pl['rows_per_wave'] > 1 and pl['lane_trips'] > 1 for c, pl in S))
    for v in ('c', 'p', 't', 'col'):
        _need(('score view', v), (c.view == v for c, pl in S))
    for nf in NF_KINDS:
        _need(('score nframes', nf), (c.nf == nf for c, pl in S))
    _need('score an empty clip among live ones, more than 16 rows', (c.nf in ('mixed', 'neg') and c.B > 16 for c, pl in S))
    for st in ('zero', 'big'):
        _need(('score start', st), (c.start == st for c, pl in S))
    _need('score increments resolved next to 1e6', (c.start == 'big' and c.nf != 'zero' for c, pl in S))
    _need('score ten calls into one acc', (c.calls == 10 and c.B > 16 for c, pl in S))
    _need('score extremes', (c.val == 'ext' and c.nf != 'zero' for c, pl in S))
    for pos in (0, 1):
        _need(('score positive', pos), (c.pos == pos for c, pl in S))
    for tg in (0.0, 0.5, 0.9):
        _need(('score target', tg), (c.target == tg for c, pl in S))


FAMILIES['score'] = Family(score_cases, score_plan, score_inputs, score_reference, score_run, score_check, score_coverage,
                           lambda c: (EXACT, REAL), True)

ORDER = ('logit', 'vec', 'sqnorm', 'commit', 'ltas', 'score')


# =====================================================================================================================
# the floor's models, the sweep, and the checks that hold for one case per family
# =====================================================================================================================
class CpuModel(object):
    """THE FLOOR'S MODELS: tests/summary_model.py and tests/eval_model.py, with what the C ABI does to a call and the models
    leave out: a cursor out of range writes nothing; the partial sums of a clip of more than 16 frames go through a slab.
    `mutate` names one mistake (tests/test_stats_fuzz_host.py)."""

    def __init__(self, mutate=None):
        self.mutate = mutate

    def logit_summary(self, cls, nframes, positive, out=None):
        return SM.logit_summary(cls, nframes, positive, out)

    def vec_stats(self, v, sign=1.0, out=None):
        return SM.vec_stats(v, sign, out)

    def sqnorm_rows(self, gx, nframes, scale, part=None, out=None, finish=True):
        return SM.sqnorm_rows(gx, nframes, scale, part, out, finish)

    def summary_commit(self, ring, cursor, cols, part=None, part_col=-1):
        if 0 <= int(cursor[0]) < ring.size(0):
            SM.summary_commit(ring, cursor, cols, part, part_col)

    def ltas_power(self, x, lens, out=None, nframes=None):
        return EM.ltas_power(x, lens, out, nframes)

    def frame_powers(self, row, n):
        """[frames, 129] fp32, as eval_model.ltas_power forms them"""
        f = EM._frames(row.detach(), n, torch.float32) * EM._WIN32
        re, im = f @ EM._COS32, f @ EM._SIN32
        return re * re + im * im

    def ltas_raw(self, x, lens, out, nframes, slab):
        """eval_model.ltas_power, and the slab rows [B, S, 129] the first launch writes: the chunks a clip has"""
        EM.ltas_power(x, lens, out, nframes)
        B, L = x.shape
        for b in range(B):
            n = L if lens is None else max(0, min(int(lens[b]), L))
            p = self.frame_powers(x[b], n)
            for q in range(cdiv(p.size(0), LT_CH)):
                slab[b, q] = p[q * LT_CH:(q + 1) * LT_CH].sum(0)

    def score_accum(self, cls, nframes, target, positive, acc):
        return EM.score_accum(cls, nframes, target, positive, acc)


def prepared(fam, ci, c, pas):
    """(inputs, float64 reference, outputs of the fp32 CPU model) of a case, built once per process and left unchanged"""
    key = (fam, ci, pas['name'])
    if key not in _CACHE:
        F = FAMILIES[fam]
        inp = F.inputs(c, pas, 1000 + ci)
        low = F.run(CpuModel(), c, pas, inp, 'cpu') if F.floor and pas is REAL else {}
        _CACHE[key] = (inp, F.reference(c, pas, inp), dict((k, v['out']) for k, v in low.items()))
    return _CACHE[key]


def generic(tag, pl, got, again):
    for k in sorted(got):
        t = (tag[0], tag[1], k)
        assert got[k]['frame_ok'], ('wrote outside its window', t)
        assert got[k]['kernel'] == pl['kernel'], ('ag_last_kernel names another kernel than the plan', t, got[k]['kernel'])
    for k in sorted(got):
        assert same(again[k]['out'], got[k]['out']), ('not reproducible', (tag[0], tag[1], k))


def sweep(fam, Kmod, device, worst=None, only=None):
    """every case of a family in its passes on `Kmod`, each run twice; ends in the family's coverage assertion (unless
    `only` filters).  worst: {kernel:output -> largest real-pass error / floor}"""
    F, seen = FAMILIES[fam], []
    for ci, (label, c) in enumerate(F.cases()):
        if only is not None and not only(label, c):
            continue
        pl = F.plan(c)
        for pas in F.passes(c):
            inp, ref, low = prepared(fam, ci, c, pas)
            got = F.run(Kmod, c, pas, inp, device)
            again = F.run(Kmod, c, pas, inp, device)
            generic((fam, label), pl, got, again)
            F.check((fam, label), c, pas, pl, inp, ref, got, low, worst)
        seen.append((label, c, pl))
    if only is None:
        F.coverage(seen)
    return seen


# one case per family for the checks that need not run on all: the precision mode, a side stream
PICK = dict(logit='25x41 p nf-neg zer pos1', vec='n257 sign', sqnorm='B5 L4100 pitch+1', commit='cap3 row1 seq9 mix',
            ltas='L4352 short pitch+7', score='33x129 t nf-mixed')


def picked(fam):
    F = FAMILIES[fam]
    ci, (label, c) = [(i, lc) for i, lc in enumerate(F.cases()) if lc[0].startswith(PICK[fam])][0]
    return F, c, prepared(fam, ci, c, REAL)[0]


def _same_outputs(a, b, what, fam):
    for k in a:
        assert same(a[k]['out'], b[k]['out']), (what, fam, k)
        assert b[k]['frame_ok'], ('wrote outside its window', fam, k)


def mode_invariant(Kmod, fam, device):
    """the bits do not depend on ag_set_precision"""
    F, c, inp = picked(fam)
    a = F.run(Kmod, c, REAL, inp, device)
    with Kmod.precision('bf16'):
        b = F.run(Kmod, c, REAL, inp, device)
    _same_outputs(a, b, 'the precision mode changed a kernel that ignores it', fam)


def side_stream(Kmod, fam, device):
    """the same bits on a side stream while the default stream is kept busy"""
    F, c, inp = picked(fam)
    a = F.run(Kmod, c, REAL, inp, device)
    busy = torch.randn(2048, 2048, device=device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        b = F.run(Kmod, c, REAL, inp, device)
    side.synchronize()
    torch.cuda.synchronize()
    _same_outputs(a, b, 'a side stream changed the bits', fam)

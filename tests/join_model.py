"""Torch-CPU fp32 model of ``audiogan_amd.kernels.join_facts`` / ``join_clips`` (ag_join_facts, ag_join_clips; contract in
include/audiogan_hip.h), the shared case table and the checkers  --  TEST INFRASTRUCTURE.

The model is written from the rule, segment by segment (each segment's weighted samples are laid over the output, a second
layer is added to the first): the launch and ``synth.join_host`` go the other way, sample by sample through a search of the
starts.  It calls neither.  Every operation of the rule is one fp32 operation rounded once, and the order of the two products
of an overlapped sample does not matter to their sum, so EVERY comparison here is bit equality: no tolerance in this file.
Every join also checks: guard floats either side, the row pitch beyond O_cap untouched, every entry of [S, O_cap] written
(the destination starts as NaN), out_len the untruncated total between its own guards."""
import collections

import numpy as np
import torch

GUARD, GUARD_VALUE = 64, 777.0
MAX_SEG = 1024
CLIP_MUTANTS = ('overlap_without_half', 'fade_index_unscaled', 'fma', 'out_len_truncated', 'pause_not_zeroed')
VALUES = ('int', 'randn')


def ramp(F):
    """the rule, stated directly: sin^2(pi (i + 0.5) / (2 F)) in float64, rounded once"""
    i = np.arange(F, dtype=np.float64)
    return torch.from_numpy((np.sin(np.pi * (i + 0.5) / (2.0 * max(F, 1))) ** 2).astype(np.float32))


def _window(off, n, L_in):
    o = min(max(int(off), 0), L_in)
    return o, min(max(int(n), 0), L_in - o)


# ----------------------------------------------------------------------------------------------------------------------
# the model of the two launches
# ----------------------------------------------------------------------------------------------------------------------
def _checks(table):
    for t, dt, what in table:
        if t is not None and t.dtype != dt:
            raise TypeError('audiogan_amd: %s must be %s, got %s' % (what, dt, t.dtype))


def join_facts(wave, off, n, target=0.0):
    _checks(((wave, torch.float32, 'wave'), (off, torch.int32, 'off'), (n, torch.int32, 'n')))
    w, R, L_in = wave.detach().cpu(), wave.size(0), wave.size(1)
    gain, bad = torch.ones(R), torch.zeros(R, dtype=torch.int32)
    tgt = torch.tensor(float(target), dtype=torch.float32)
    for r in range(R):
        o, m = _window(off[r], n[r], L_in)
        bits = w[r, o:o + m].contiguous().view(torch.int32) & 0x7fffffff
        top = int(bits.max()) if m else 0
        if top >= 0x7f800000:
            gain[r], bad[r] = 0.0, 1
        elif float(target) > 0 and top > 0:
            gain[r] = tgt / torch.tensor([top], dtype=torch.int32).view(torch.float32)[0]
    return gain.to(wave.device), bad.to(wave.device)


def join_clips(wave, off, n, gain, seg_row, join, sent_ptr, ramp, out, out_len=None, pause_max=0, mutate=None):
    _checks(((wave, torch.float32, 'wave'), (off, torch.int32, 'off'), (n, torch.int32, 'n'), (gain, torch.float32, 'gain'),
             (seg_row, torch.int32, 'seg_row'), (join, torch.int32, 'join'), (sent_ptr, torch.int32, 'sent_ptr'),
             (ramp, torch.float32, 'ramp'), (out, torch.float32, 'out'), (out_len, torch.int64, 'out_len')))
    w, g, rp = wave.detach().cpu(), gain.detach().cpu(), ramp.detach().cpu()
    offs, ns, rows, jn, sp = (t.cpu().tolist() for t in (off, n, seg_row, join, sent_ptr))
    R, L_in, F = w.size(0), w.size(1), rp.numel()
    S, O = len(sp) - 1, out.size(1)
    if out.dim() != 2 or out.size(0) != S:
        raise ValueError('audiogan_amd: out must be [%d, O_cap]' % S)
    res, lens = torch.zeros(S, O), []
    for s in range(S):
        ks = list(range(sp[s], sp[s + 1]))[:MAX_SEG]
        segs = [(rows[k],) + _window(offs[rows[k]], ns[rows[k]], L_in) if 0 <= rows[k] < R else (0, 0, 0) for k in ks]
        st, at = [], 0
        for i, (_, _, m) in enumerate(segs):
            st.append(at)
            at += m
            if i + 1 < len(segs):
                j, nxt = jn[ks[i]], segs[i + 1][2]
                if j >= 0:
                    at += min(j, int(pause_max))
                else:
                    at -= min(-j, min(m, nxt) if mutate == 'overlap_without_half' else min(m // 2, nxt // 2))
        total = at
        val = torch.full((O,), float('nan')) if mutate == 'pause_not_zeroed' else torch.zeros(O)
        val[total:] = 0
        prod64 = torch.zeros(O, dtype=torch.float64)
        cover = torch.zeros(O, dtype=torch.int64)
        for i, (row, o, m) in enumerate(segs):
            a, b = st[i], min(st[i] + m, O)
            if m == 0 or a >= O:
                continue
            f = min(F, m // 2)
            idx = torch.arange(m)
            wt = torch.ones(m)
            if f > 0:
                wt[:f] = rp[idx[:f] if mutate == 'fade_index_unscaled' else (idx[:f] * F) // f]
                wt[m - f:] = rp[m - 1 - idx[m - f:] if mutate == 'fade_index_unscaled' else ((m - 1 - idx[m - f:]) * F) // f]
            c = g[row] * wt                              # fp32: one product
            x = w[row, o:o + m]
            y = (x * c)[:b - a]                          # fp32: one product
            first = cover[a:b] == 0
            assert bool((cover[a:b] <= 1).all()), 'three segments over one sample'
            if mutate == 'fma':                          # the earlier product unrounded inside the sum
                both = (prod64[a:b] + y.double()).float()
            else:
                both = val[a:b] + y                      # fp32: one sum
            val[a:b] = torch.where(first, y, both)
            prod64[a:b] = (x.double() * c.double())[:b - a]
            cover[a:b] += 1
        res[s] = val
        lens.append(min(total, O) if mutate == 'out_len_truncated' else total)
    out.copy_(res.to(out.device))
    if out_len is None:
        out_len = torch.empty(S, dtype=torch.int64, device=out.device)
    out_len.copy_(torch.tensor(lens, dtype=torch.int64).reshape(S))
    return out, out_len


# ----------------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'name reason L_in off n sents F O_cap pitch shift unit_gain')


def _case(name, reason, L_in, n, sents, F, O_cap, off=None, pitch=None, shift=0, unit_gain=False):
    """``sents``: per sentence a list of (row, join); ``pitch`` None: O_cap rounded up to 4 floats (the 16-byte form)"""
    off = [0] * len(n) if off is None else off
    return Case(name, reason, L_in, list(off), list(n), sents, F, O_cap, pitch if pitch is not None else (O_cap + 3) // 4 * 4,
                shift, unit_gain)


def _chain(rows, join):
    return [(r, join) for r in rows]


def clip_cases():
    rs = np.random.RandomState(23)
    c = []
    c.append(_case('plain', 'one segment, n = 5, no fade, gain 1: a copy', 8, [5], [[(0, 0)]], 0, 8, unit_gain=True))
    c.append(_case('fade_clip', 'n of 0, 1, 2, 3, 9 and 5 with F = 4: the fade clipped to n / 2; n = 5: f_k = 2, (i F) / f_k != i', 12,
                   [0, 1, 2, 3, 9, 5], [_chain(range(6), 2)], 4, 36))
    c.append(_case('overlap_edge', 'n = (1040, 100), join -40: the overlap 1000..1039 straddles output 1024', 1040,
                   [1040, 100], [_chain([0, 1], -40)], 8, 1104))
    c.append(_case('pause_edge', 'n = (1020, 30), a pause of 10: zeros over 1020..1029 straddle 1024', 1020,
                   [1020, 30], [_chain([0, 1], 10)], 8, 1064))
    c.append(_case('ov_clamps', 'join -50 with n = (13, 40): ov 6; (40, 1): ov 0; (40, 0, 40): no overlap across an empty one', 40,
                   [13, 40, 1, 0], [_chain([0, 1], -50), _chain([1, 2], -50), _chain([1, 3, 1], -50)], 3, 96))
    c.append(_case('empty_segs', 'empty segments first, middle and last; an empty sentence between two others', 9,
                   [0, 7, 9], [_chain([0, 1, 0, 2, 0], 3), [], _chain([0, 2, 0, 0, 1], -2)], 2, 36))
    n300 = rs.randint(0, 8, 300).tolist()
    c.append(_case('scan300', '300 segments of n in 0..7, pauses and overlaps: the scan crosses threads and waves', 7, n300,
                   [[(r, int(rs.randint(-3, 4))) for r in range(300)]], 2, 2048))
    n1024 = rs.randint(0, 8, 1024).tolist()
    c.append(_case('scan1024', 'exactly 1024 segments: every slot of the scan', 7, n1024,
                   [[(r, int(rs.randint(-3, 3))) for r in range(1024)]], 1, 4100))
    c.append(_case('shared_rows', 'three sentences that share rows; one row twice in a sentence', 33, [33, 20, 11, 5],
                   [_chain([0, 1, 0], -6), _chain([1, 2, 3, 1], 4), _chain([3, 0], -2)], 5, 120))
    c.append(_case('windows', 'off of 1, 2, 3 and -2; off + n > L_in; a negative n; off > L_in', 30,
                   [20, 20, 20, 40, -5, 28, 4], [_chain([0, 1, 2, 3, 4, 5, 6], -4), _chain([3, 5], 1)], 3, 160,
                   off=[1, 2, 3, -2, 4, 7, 31]))
    for O in (1023, 1024, 1027):
        c.append(_case('ocap%d' % O, 'O_cap = %d against a total of 1100: the last group of a row, a cropped sentence' % O,
                       600, [600, 560], [_chain([0, 1], -60), _chain([1], 0)], 16, O))
    c.append(_case('odd_pitch', 'an out view at an odd pitch, 4 bytes off a 16-byte boundary: the scalar stores', 600,
                   [600, 560], [_chain([0, 1], -60), _chain([1], 0)], 16, 1027, pitch=1029, shift=1))
    c.append(_case('truncated', 'O_cap < total: out_len is the total, the written part the sentence\'s start', 50,
                   [50, 50, 50], [_chain([0, 1, 2], 5)], 4, 77))
    c.append(_case('long_ramp', 'F = 4096 with n = 8192: the longest ramp, a constant-gain crossfade of two clips', 8192,
                   [8192, 8192], [_chain([0, 1], -4096)], 4096, 12288))
    return c


def _values(case, values):
    """-> (wave [R, L_in], gain [R]): integer-valued samples with power-of-two gains (outside the fades every product and sum
    is exact: a wrong index or plan shows whatever the roundings do), or normal samples with arbitrary gains (every rounding
    shows)"""
    rs = np.random.RandomState(sum(map(ord, case.name)))
    R = len(case.n)
    if values == 'int':
        wave = rs.randint(-9, 10, (R, case.L_in)).astype(np.float32)
        wave[wave == 0] = 1
        gain = np.float32(2.0) ** rs.randint(-2, 3, R).astype(np.float32)
    else:
        wave = rs.randn(R, case.L_in).astype(np.float32)
        gain = rs.uniform(0.5, 1.5, R).astype(np.float32)
    if case.unit_gain:
        gain[:] = 1
    return torch.from_numpy(wave), torch.from_numpy(gain)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_WANT = {}


def _expected(case, values):
    """the model's answer, computed once per (case, values) and never changed"""
    key = (case.name, values)
    if key not in _WANT:
        args = _args(case, values)
        out = torch.full((len(case.sents), case.O_cap), float('nan'))
        ln = torch.zeros(len(case.sents), dtype=torch.int64)
        join_clips(*args[:8], out, ln, pause_max=args[8])
        _WANT[key] = (out, ln)
    return _WANT[key]


def _args(case, values, on=lambda t: t):
    wave, gain = _values(case, values)
    i32 = lambda v: on(torch.tensor(v, dtype=torch.int32))          # noqa: E731
    seg_row = [r for s in case.sents for r, _ in s]
    join = [j for s in case.sents for _, j in s]
    sent_ptr = np.concatenate([[0], np.cumsum([len(s) for s in case.sents])]).tolist()
    return (on(wave), i32(case.off), i32(case.n), on(gain), i32(seg_row), i32(join), i32(sent_ptr), on(ramp(case.F)),
            max([j for j in join if j > 0] + [0]))


def run_clips(fn, case, values, on=lambda t: t, form=None):
    """one join under every check.  ``fn``: the wrapper's signature.  ``form``: None - the case's own pitch and shift;
    'scalar' - an odd pitch one float off a 16-byte boundary; 'vector' - an aligned one.  -> the rows written"""
    S, O = len(case.sents), case.O_cap
    pitch, shift = {None: (case.pitch, case.shift), 'scalar': (O + 1 + O % 2, 1), 'vector': ((O + 3) // 4 * 4, 0)}[form]
    args = _args(case, values, on)
    flat = on(torch.full((shift + S * pitch + 2 * GUARD,), float('nan')))
    flat[:GUARD + shift] = GUARD_VALUE
    flat[GUARD + shift + S * pitch:] = GUARD_VALUE
    before = _bits(flat).clone()
    lo, hi = GUARD + shift, GUARD + shift + S * pitch
    out = flat[lo:hi].view(S, pitch)[:, :O]
    ln = on(torch.full((S + 2,), -5, dtype=torch.int64))
    got, got_len = fn(*args[:8], out, ln[1:S + 1], pause_max=args[8])
    assert got is out
    now = _bits(flat)
    assert torch.equal(now[:lo], before[:lo]) and torch.equal(now[hi:], before[hi:]), ('guards', case.name)
    assert torch.equal(now[lo:hi].view(S, pitch)[:, O:], before[lo:hi].view(S, pitch)[:, O:]), ('the pitch', case.name)
    rows = out.detach().cpu()
    assert not torch.isnan(rows).any(), ('every entry of [S, O_cap] is written', case.name, int(torch.isnan(rows).sum()))
    want, want_len = _expected(case, values)
    lens = ln.cpu()
    assert lens[0] == -5 and lens[-1] == -5, ('length guards', case.name)
    assert torch.equal(lens[1:S + 1], want_len), ('out_len', case.name, lens[1:S + 1].tolist(), want_len.tolist())
    assert torch.equal(_bits(rows), _bits(want)), ('out', case.name, values, int((_bits(rows) != _bits(want)).sum()))
    return rows


def check_clips(fn, on=lambda t: t, forms=(None,)):
    for values in VALUES:
        for case in clip_cases():
            for form in forms:
                run_clips(fn, case, values, on, form)
    return len(clip_cases())


def facts_rows():
    """(wave [R, 16], off, n, reasons)"""
    nan, inf = float('nan'), float('inf')
    z = [0.0] * 16
    rows = [
        (z, 2, 9, 'an all-zero row: gain 1'),
        ([9.0, 8.0, 0.5, -0.75, 0.25] + [0.0] * 6 + [7.0] * 5, 2, 9, 'larger samples just outside the window either side'),
        ([0.5, 0.25, nan, 0.125] + [0.0] * 12, 0, 4, 'a NaN in the window: bad'),
        ([0.5, -inf, 0.25] + [0.0] * 13, 1, 2, 'an infinity in the window: bad'),
        ([nan, 0.5, -0.5, inf] + [0.0] * 12, 1, 2, 'a NaN and an infinity just outside the window: not bad'),
        ([3.0] * 16, 5, 0, 'n = 0: peak 0, gain 1'),
        ([0.1 * (i - 7) for i in range(16)], 3, 40, 'off + n beyond the row: the window is cropped'),
        ([1.0 + i for i in range(16)], -3, 6, 'a negative off: clamped to 0'),
    ]
    wave = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    return wave, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]


def check_facts(fn, on=lambda t: t):
    """gain and bad of every row at a target of 0.9 and of 0 against the model, bit for bit"""
    wave, off, n, reasons = facts_rows()
    a = (on(wave), on(torch.tensor(off, dtype=torch.int32)), on(torch.tensor(n, dtype=torch.int32)))
    for target in (0.9, 0.0):
        gain, bad = fn(*a, target)
        assert gain.dtype == torch.float32 and bad.dtype == torch.int32 and tuple(gain.shape) == tuple(bad.shape) == (len(n),)
        wg, wb = join_facts(wave, *(t.cpu() for t in a[1:]), target)
        assert wb.tolist() == [0, 0, 1, 1, 0, 0, 0, 0]
        assert torch.equal(bad.cpu(), wb), ('bad', target, bad.tolist())
        assert torch.equal(_bits(gain), _bits(wg)), ('gain', target, gain.tolist(), wg.tolist())
        if target == 0.0:
            assert gain.cpu().tolist() == [1, 1, 0, 0, 1, 1, 1, 1]
    return len(n)


ALL = ('join_facts', 'join_clips')


def install(monkeypatch):
    """the CPU model of both launches in the wrappers' place"""
    import audiogan_amd.kernels as K
    for name in ALL:
        assert hasattr(K, name), 'join model has %s but audiogan_amd.kernels does not' % name
        monkeypatch.setattr(K, name, globals()[name])

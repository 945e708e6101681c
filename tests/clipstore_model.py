"""Torch-CPU model of ``audiogan_amd.kernels.clip_facts`` / ``clip_gather`` (ag_clip_facts, ag_clip_gather; contract in
include/audiogan_hip.h), the host rule they must reproduce, the shared case table and the checkers  --  TEST INFRASTRUCTURE.

The reference is the host loader itself (``dataset.pick_word`` followed by ``tovar``'s float32 cast): the length is the index
after the last non-zero sample (``ingest.clip_length``), the row is the clip divided by its peak in float64, cast to float32
and zero padded.  For float32 operands that is the correctly rounded float32 quotient (53 >= 2 * 24 + 2), and n and the peak
are order-independent, so EVERY comparison here is bit equality: there is no tolerance anywhere in this file.
Every gather also checks: guard floats either side, the row pitch beyond the row's width untouched, every entry of the
width written (the destination starts as NaN), lengths rounded up to the frame and not cropped."""
import collections

import numpy as np
import torch

from audiogan_amd import ingest

GUARD, GUARD_VALUE = 64, 777.0
MAXLEN, FRAME = 48, 8          # the loader tests' clip length and frame: 'long' does not fit, 'zero' holds a silent clip
FACT_MUTANTS = ('n_off_by_one', 'nan_dropping_max')
GATHER_MUTANTS = ('reciprocal', 'length_unrounded', 'no_zero_fill')
DEN = np.float32(1e-40)          # a denormal float32


def _clip(width, values, at=0):
    x = np.zeros(width, dtype=np.float32)
    x[at:at + len(values)] = values
    return x


def words():
    """word -> [(clip, reason)]: the clips of a word share its row width (maxlen_word)"""
    rs = np.random.RandomState(11)
    u = lambda n: rs.uniform(-1, 1, n).astype(np.float32)          # noqa: E731
    w = collections.OrderedDict()
    w['zero'] = [(_clip(8, []), 'n = 0: all zero, a silent clip - the loader redraws'),
                 (_clip(8, u(6)), 'an audible clip of the same word')]
    w['tiny'] = [(_clip(5, u(1)), 'n = 1'), (_clip(5, u(3)), 'n = 3: inside the first 16-byte group'),
                 (_clip(5, u(4)), 'n = 4: one whole group'), (_clip(5, u(5)), 'n = 5 = cap: a width that is no multiple of 4')]
    holes = u(30)
    holes[[3, 4, 5, 17, 28]] = 0
    w['holes'] = [(_clip(40, holes), 'interior zeros: the length is after the LAST non-zero sample'),
                  (_clip(40, np.concatenate([u(20), np.full(9, -0.0, np.float32)])), 'a tail of -0.0: zero, n = 20'),
                  (_clip(40, np.concatenate([u(20), [0, 0, DEN]])), 'a denormal last sample: not zero, n = 23')]
    w['denpk'] = [(_clip(12, np.array([3, -7, 2, 5, -1, 6, 4], np.float32) * DEN), 'a denormal peak: quotients of denormals')]
    w['long'] = [(_clip(1100, u(1100)), 'n = 1100 = cap: longer than the loaders\' maxlen, cropped by a width below n'),
                 (_clip(1100, u(1000)), 'n = 1000: more than one tile of 1024 with the row above; random quotients')]
    w['single'] = [(_clip(41, u(37)), 'a word with one clip')]
    for i, name in enumerate(('alpha', 'beta', 'gamma', 'delta', 'epsil', 'zetaa')):
        w[name] = [(_clip(43 + i, u(9 + 5 * k + i)), 'plain clips, odd widths') for k in range(1 + i % 3)]
    w['omega'] = [(_clip(7, u(2)), 'n = 2'), (_clip(7, u(7)), 'the last clip of the bank, n = cap = 7: its last group ends the bank')]
    return w


def mapping(table=None):
    """the word store layout: word -> float32 [n_clips, maxlen_word]"""
    return collections.OrderedDict((k, np.stack([c for c, _ in v])) for k, v in (table or words()).items())


def special():
    """facts only (a store refuses them): NaN and infinite samples"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    return collections.OrderedDict(
        nan=[(_clip(9, np.array([0.5, nan, 0.25], np.float32)), 'a NaN inside: the peak is NaN'),
             (_clip(9, np.array([0.5, 0, 0, 0, 0, 0, nan], np.float32)), 'a NaN last: not zero, n = 7'),
             (_clip(9, np.array([nan, 3.0, -4.0], np.float32)), 'a NaN first, larger values after it')],
        inf=[(_clip(6, np.array([1.0, -inf, 2.0], np.float32)), 'an infinite sample: the peak is +inf')])


def pack(m):
    """the packed layout, stated directly -> (bank float32, start int64, cap int32, clips [(word, row, array)])"""
    clips = [(w, i, np.asarray(m[w][i], dtype=np.float32)) for w in m for i in range(m[w].shape[0])]
    start, at = [], 0
    for _, _, c in clips:
        start.append(at)
        at += (len(c) + 3) // 4 * 4
    bank = np.zeros(at, dtype=np.float32)
    for s, (_, _, c) in zip(start, clips):
        bank[s:s + len(c)] = c
    return bank, np.asarray(start, dtype=np.int64), np.asarray([len(c) for _, _, c in clips], dtype=np.int32), clips


def host_row(clip, width, frame=None):
    """dataset.pick_word + tovar for one clip at a row of ``width`` -> (float32 row, length as the loader reports it)"""
    n = ingest.clip_length(clip)
    row = np.zeros(max(n, width))          # float64, as the loader's NP.zeros(maxlen)
    row[:n] = clip[:n]
    if n:
        row /= np.abs(row).max()
    return row[:width].astype(np.float32), (n if not frame else (n + frame - 1) // frame * frame)


def _bits(t):
    t = t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def check_facts(fn, on=lambda t: t, with_special=True):
    """n and peak of every clip of the table (and of the NaN / infinite clips) against ingest.clip_length and abs().max()"""
    table = words()
    if with_special:
        table.update(special())
    bank, start, cap, clips = pack(mapping(table))
    n, peak = fn(on(torch.from_numpy(bank)), on(torch.from_numpy(start)), on(torch.from_numpy(cap)))
    assert n.dtype == torch.int32 and peak.dtype == torch.float32 and tuple(n.shape) == tuple(peak.shape) == (len(clips),)
    n, peak = n.cpu().numpy(), peak.cpu().numpy()
    for c, (w, i, x) in enumerate(clips):
        want_n, want_p = ingest.clip_length(x), (np.abs(x).max() if len(x) else np.float32(0))
        assert int(n[c]) == want_n, ('n', w, i, int(n[c]), want_n)
        if np.isnan(want_p):
            assert np.isnan(peak[c]), ('a NaN peak', w, i, peak[c])
        else:
            assert peak[c].view(np.int32) == np.float32(want_p).view(np.int32), ('peak', w, i, peak[c], want_p)
    return len(clips)


def gather_cases():
    """(ids, width, pitch, offset in floats of row 0 from a 16-byte boundary, frame, reason); ids index pack(mapping())"""
    _, _, _, clips = pack(mapping())
    at = {(w, i): c for c, (w, i, _) in enumerate(clips)}
    every = list(range(len(clips)))
    last = len(clips) - 1
    out = []
    for width in (40, 41, 43, 1027):
        out.append((every, width, width + (4 - width % 4) % 4, 0, FRAME, 'every clip at width %d, 16-byte rows' % width))
    out += [
        (every, 41, 41, 0, None, 'an odd pitch: rows 1.. are misaligned - the scalar path'),
        (every, 40, 44, 1, FRAME, 'out offset by one float: the scalar path at an even width'),
        (every, 43, 64, 0, 200, 'ld_out > L_out, the reference\'s frame of 200'),
        ([at['long', 0]], 1027, 1028, 0, FRAME, 'B = 1, a width below the clip\'s n = 1100: cropped, length not'),
        ([at['long', 1], at['long', 0], at['long', 1]], 1000, 1000, 0, 256, 'B = 3, a width equal to n, a repeated id'),
        ([last, last, at['tiny', 3]], 5, 8, 0, 4, 'B = 3: the last clip of the bank twice, n = cap = width'),
        ([last], 1, 1, 3, None, 'B = 1, one column, misaligned'),
        ([every[i % len(every)] for i in range(64)], 43, 44, 0, FRAME, 'B = 64: repeated ids'),
        ([at['long', i % 2] for i in range(64)], 1027, 1027, 0, FRAME, 'B = 64 at an odd width and pitch: two tiles a row'),
    ]
    return out


def run_gather(fn, case, on=lambda t: t, store=None):
    """one gather under every check -> (rows float32 [B, width] numpy, ids)"""
    ids, width, pitch, off, frame, reason = case
    bank, start, cap, clips = pack(mapping())
    if store is None:
        n = np.asarray([ingest.clip_length(c) for _, _, c in clips], dtype=np.int32)
        peak = np.asarray([np.abs(c).max() for _, _, c in clips], dtype=np.float32)
        store = tuple(on(torch.from_numpy(a)) for a in (bank, start, n, peak))
    B = len(ids)
    flat = on(torch.full((off + B * pitch + 2 * GUARD,), float('nan')))
    flat[:GUARD + off] = GUARD_VALUE
    flat[GUARD + off + B * pitch:] = GUARD_VALUE
    before = _bits(flat).clone()
    out = flat[GUARD + off:GUARD + off + B * pitch].view(B, pitch)[:, :width]
    ln = on(torch.full((B + 2,), -5, dtype=torch.int64))
    got, got_len = fn(*store, on(torch.tensor(ids, dtype=torch.int64)), out, ln[1:B + 1], frame or 0)
    assert got is out
    now = _bits(flat)
    lo, hi = GUARD + off, GUARD + off + B * pitch
    assert torch.equal(now[:lo], before[:lo]) and torch.equal(now[hi:], before[hi:]), ('guards', reason)
    assert torch.equal(now[lo:hi].view(B, pitch)[:, width:], before[lo:hi].view(B, pitch)[:, width:]), ('the pitch', reason)
    rows = out.detach().cpu().numpy()
    assert not np.isnan(rows).any(), ('every entry of the width is written', reason)
    lens = ln.cpu().tolist()
    assert lens[0] == lens[-1] == -5, ('length guards', reason)
    for b, c in enumerate(ids):
        want, want_len = host_row(clips[c][2], width, frame)
        assert np.array_equal(rows[b].view(np.int32), want.view(np.int32)), \
            ('row', reason, b, clips[c][:2], int((rows[b].view(np.int32) != want.view(np.int32)).sum()))
        assert lens[1 + b] == want_len, ('length', reason, b, lens[1 + b], want_len)
    return rows, ids


def check_gather(fn, on=lambda t: t):
    for case in gather_cases():
        run_gather(fn, case, on)
    return len(gather_cases())


# ----------------------------------------------------------------------------------------------------------------------
# the model of the two launches
# ----------------------------------------------------------------------------------------------------------------------
def _store_checks(bank, start, second, name):
    for t, dt, what in ((bank, torch.float32, 'bank'), (start, torch.int64, 'start'), (second, torch.int32, name)):
        if t.dtype != dt:
            raise TypeError('audiogan_amd: %s must be %s, got %s' % (what, dt, t.dtype))
    if bank.dim() != 1 or bank.numel() % 4 or tuple(second.shape) != tuple(start.shape) or start.dim() != 1:
        raise ValueError('audiogan_amd: the clip bank must be 1-D and a multiple of 4 floats long, start and %s vectors' % name)


def clip_facts(bank, start, cap, mutate=None):
    _store_checks(bank, start, cap, 'cap')
    bk, st, cp = bank.detach().cpu().numpy(), start.cpu().numpy(), cap.cpu().numpy()
    assert (st % 4 == 0).all()
    n, peak = np.zeros(len(st), np.int32), np.zeros(len(st), np.float32)
    for c in range(len(st)):
        x = bk[st[c]:st[c] + cp[c]]
        a = x.view(np.uint32) & np.uint32(0x7fffffff)          # |x| as bits: a denormal is not zero whatever the float mode
        nz = np.nonzero(a)[0]
        n[c] = (int(nz[-1]) + 1 if len(nz) else 0) - (1 if mutate == 'n_off_by_one' and len(nz) else 0)
        if mutate == 'nan_dropping_max':
            peak[c] = np.fmax.reduce(np.abs(x)) if len(x) else 0
        else:
            peak[c] = (a.max() if len(a) else np.uint32(0)).view(np.float32)
    return torch.from_numpy(n).to(bank.device), torch.from_numpy(peak).to(bank.device)


def clip_gather(bank, start, n, peak, ids, out, len_out=None, frame=0, mutate=None):
    _store_checks(bank, start, n, 'n')
    for t, dt, what in ((peak, torch.float32, 'peak'), (ids, torch.int64, 'ids'), (out, torch.float32, 'out'),
                        (len_out, torch.int64, 'len_out')):
        if t is not None and t.dtype != dt:
            raise TypeError('audiogan_amd: %s must be %s, got %s' % (what, dt, t.dtype))
    B = ids.numel()
    if out.dim() != 2 or out.size(0) != B or (out.size(1) > 1 and out.stride(1) != 1):
        raise ValueError('audiogan_amd: out must be [%d, W] with unit stride along W' % B)
    W = out.size(1)
    if B > 1 and out.stride(0) < W:
        raise ValueError('ag_clip_gather: rows of %d samples at a pitch of %d' % (W, out.stride(0)))
    bk, st, nn, pk = bank.detach().cpu().numpy(), start.cpu().numpy(), n.cpu().numpy(), peak.cpu().numpy()
    frame = int(frame or 0)
    for b, c in enumerate(ids.cpu().tolist()):
        assert 0 <= c < len(st), 'the caller\'s duty'
        m = min(int(nn[c]), W)
        x = bk[st[c]:st[c] + m]
        with np.errstate(all='ignore'):
            q = x * (np.float32(1) / pk[c]) if mutate == 'reciprocal' else x / pk[c]          # float32: correctly rounded
        out[b, :m] = torch.from_numpy(q.astype(np.float32)).to(out.device)
        if mutate != 'no_zero_fill':
            out[b, m:] = 0
        if len_out is not None:
            k = int(nn[c])
            len_out[b] = k if (frame <= 0 or mutate == 'length_unrounded') else (k + frame - 1) // frame * frame
    return out, len_out


def loop_setup(A, dev, wide, B, device_store=None, seed=5):
    """models, optimisers and loaders as tests/test_loop.py sets them up (``wide``: its C2 widths), the loader over a
    DeviceWordStore on ``device_store`` when that is given -> (make TrainLoop(**kw), modules, validation loader, maxlen)"""
    import types
    from audiogan_amd import dataset as D, loop, optim
    torch.manual_seed(81)
    if wide:
        frame, maxlen = 256, 8192
        gcfg = dict(frame_size=frame, embed_size=100, noise_size=100, state_size=1024, num_layers=1)
        dcfg = dict(state_size=1024, embed_size=100, num_layers=1)
        ecfg = dict(output_size=100, char_embed_size=50, num_layers=1, num_chars=256)
    else:
        frame, maxlen = 32, 128
        gcfg = dict(frame_size=frame, embed_size=8, noise_size=8, state_size=64, num_layers=1, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])
        dcfg = dict(state_size=64, embed_size=8, num_layers=1, cnn_struct=[[7, 2, 8], [7, 2, 16]])
        ecfg = dict(output_size=8, char_embed_size=6, num_chars=256)
    g, d = A.Generator(**gcfg).to(dev), A.Discriminator(**dcfg).to(dev)
    e_g, e_d = A.Embedder(**ecfg).to(dev), A.Embedder(**ecfg).to(dev)
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    names = ['alpha', 'beta', 'gamma', 'delta', 'epsil', 'zetaa', 'etaaa', 'theta', 'iotaa', 'kappa', 'lambd']
    ds = D.SyntheticWordDataset(names, n_per_word=3, min_len=maxlen // 3, max_len=maxlen, kind='noise', seed=3)
    args = types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0)
    if device_store is not None:
        args.device_store = device_store
    np.random.seed(seed)
    h5, ml, gen_train, gen_val, keys_train, _ = D.dataloader(B, args, maxlen=maxlen, frame_size=frame)
    assert isinstance(h5, D.DeviceWordStore) == (device_store is not None)
    pick = loop.words_picker(D, B, ml, h5, keys_train, args, frame_size=frame)
    mk = lambda **kw: loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, ml, dev, **kw)  # noqa: E731
    return mk, (g, d, e_g, e_d), gen_val, ml


def run_both_loaders(A, dev, wide, B, passes, **kw):
    """``passes`` of TrainLoop.outer with the host loader and with the device loader from the same seeds -> the two
    parameter lists (to be compared with torch.equal) and the two loops"""
    res = []
    for device_store in (None, dev):
        mk, mods, _, _ = loop_setup(A, dev, wide, B, device_store)
        torch.manual_seed(17)
        lp = mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, host=False, **kw)
        for _ in range(passes):
            lp.outer()
        assert lp._clips == (device_store is not None)
        res.append(([p.detach().clone() for m in mods for p in m.parameters()], lp))
    return res


ALL = ('clip_facts', 'clip_gather')


def install(monkeypatch):
    """the CPU model of both launches in the wrappers' place (after ``kernel_model.install`` where both are used)"""
    import audiogan_amd.kernels as K
    for name in ALL:
        assert hasattr(K, name), 'clip store model has %s but audiogan_amd.kernels does not' % name
        monkeypatch.setattr(K, name, globals()[name])

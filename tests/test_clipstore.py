"""The device-resident word store on the CPU: the packing of dataset.DeviceWordStore, the model of ag_clip_facts / ag_clip_gather
(tests/clipstore_model.py) under the GPU checkers and the mutants they must reject, store.pick_words / device_dataloader
against the host loader at the same seed, train.Feeder(clips=...), the refusals.  The model stands for the launch here;
-m gpu: tests/test_gpu_clipstore.py.  Every comparison is bit equality (the module text of tests/clipstore_model.py)."""
import os
import types

import numpy as np
import pytest
import torch

from audiogan_amd import dataset as D
from audiogan_amd import ingest
from tests import clipstore_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def store(monkeypatch):
    M.install(monkeypatch)
    return D.DeviceWordStore(M.mapping(), 'cpu', piece=64)          # (a small piece: clips straddle the upload buffer)


def _args(ds, **kw):
    return types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0, **kw)


def test_packing_facts(store):
    bank, start, cap, clips = M.pack(M.mapping())
    assert store.n_clips == len(clips) and store.keys() == list(M.mapping())
    assert store.bank.numel() % 4 == 0 and (store.start_host % 4 == 0).all() and store.bank.data_ptr() % 16 == 0
    assert np.array_equal(store.start_host, start) and np.array_equal(store.cap_host, cap)
    assert store.start.dtype == torch.int64 and store.cap.dtype == torch.int32
    assert torch.equal(store.bank.view(torch.int32), torch.from_numpy(bank).view(torch.int32))          # order, zero padding
    got = store.bank.numpy()
    for c, (w, i, x) in enumerate(clips):
        assert store._first[w] + i == c and store[w].shape == M.mapping()[w].shape
        assert np.array_equal(got[start[c]:start[c] + cap[c]].view(np.int32), x.view(np.int32))
        end = start[c + 1] if c + 1 < len(clips) else len(got)
        assert not got[start[c] + cap[c]:end].view(np.int32).any()
    # one piece for the whole bank, and a piece smaller than a clip, give the same bank
    for piece in (1 << 20, 8):
        other = D.DeviceWordStore(M.mapping(), 'cpu', piece=piece)
        assert torch.equal(other.bank.view(torch.int32), store.bank.view(torch.int32))


def test_facts_equal_the_loaders_rule(store):
    assert M.check_facts(M.clip_facts) == store.n_clips + 4
    _, _, _, clips = M.pack(M.mapping())
    for c, (w, i, x) in enumerate(clips):
        assert store.n[c] == ingest.clip_length(x) and bool(store.silent[c]) == (not x.any())
        assert float(store.peak[c]) == float(np.abs(x).max())
    assert store.silent.sum() == 1


def test_model_gather_against_the_host_rule():
    assert M.check_gather(M.clip_gather) == len(M.gather_cases())


@pytest.mark.parametrize('mutant', M.FACT_MUTANTS + M.GATHER_MUTANTS)
def test_checkers_reject_mutants(mutant):
    if mutant in M.FACT_MUTANTS:
        with pytest.raises(AssertionError):
            M.check_facts(lambda *a: M.clip_facts(*a, mutate=mutant))
        return
    fn = lambda *a: M.clip_gather(*a, mutate=mutant)          # noqa: E731
    if mutant == 'reciprocal':          # the data on which x * (1 / p) is not x / p: 2100 random quotients of the 'long' word
        bank, start, cap, clips = M.pack(M.mapping())
        (c,) = [k for k, (w, i, _) in enumerate(clips) if (w, i) == ('long', 0)]
        x = clips[c][2]
        p = np.abs(x).max()
        differ = int((x * (np.float32(1) / p) != x / p).sum())
        print('reciprocal multiply differs from the division on %d of %d samples' % (differ, len(x)))
        assert differ > 20
    with pytest.raises(AssertionError):
        M.check_gather(fn)


def _same_picks(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), (x, y)


def test_pick_words_against_the_host_function(store, monkeypatch):
    ds = M.mapping()
    keys = list(ds)
    mc = max(len(k) for k in keys)
    calls = []
    choice = D.RNG.choice
    monkeypatch.setattr(D.RNG, 'choice', lambda *a, **k: calls.append(1) or choice(*a, **k))
    for frame, skip, B, sub in ((M.FRAME, False, 64, keys), (None, False, 3, keys), (M.FRAME, True, 5, keys),
                                (M.FRAME, False, 8, ['long', 'single']), (M.FRAME, False, 8, ['zero', 'single'])):
        np.random.seed(21)
        del calls[:]
        hk, hs, hl, hx, hn = D.pick_words(B, M.MAXLEN, ds, sub, mc, None, frame_size=frame, skip_samples=skip)
        host_calls, state = len(calls), np.random.get_state()
        np.random.seed(21)
        del calls[:]
        dk, dsq, dl, batch, dn = store.pick_words(B, M.MAXLEN, sub, mc, frame_size=frame, skip_samples=skip)
        assert len(calls) == host_calls and (skip or len(sub) > 2 or host_calls > 2 * B)          # both redraw paths are reached
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        _same_picks((hk, hs, hl, hn), (dk, dsq, dl, dn))
        assert isinstance(batch, D.ClipBatch) and batch.shape == hx.shape == (B, M.MAXLEN)
        got = np.asarray(batch)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), hx.astype(np.float32).view(np.int32))
        assert np.array_equal(batch[:, :7], got[:, :7]) and np.asarray(batch) is got          # one gather, one read
        assert np.array_equal(np.ascontiguousarray(batch, dtype=np.float32), got)
        # a narrower out crops, a wider one is zero-filled; lengths are the loader's
        for W in (1, 31, M.MAXLEN + 9):
            out, ln = batch.gather(torch.full((B, W), float('nan')), torch.zeros(B, dtype=torch.int64))
            want = np.zeros((B, W), np.float32)
            want[:, :min(W, M.MAXLEN)] = got[:, :W]
            assert np.array_equal(out.numpy().view(np.int32), want.view(np.int32)) and ln.tolist() == list(hn)


def test_device_dataloader_against_conditional_dataloader(monkeypatch):
    M.install(monkeypatch)
    ds = M.mapping()
    ds['(noise)'] = np.ones((1, 4), np.float32)          # filtered keys stay in the store, never in the split
    ds['cut-'] = np.ones((1, 4), np.float32)
    for maxlen in (M.MAXLEN, None):
        np.random.seed(8)
        h5, hm, htrain, hval, hkt, hkv = D.dataloader(4, _args(ds), maxlen=maxlen, frame_size=M.FRAME)
        host = [next(htrain) for _ in range(3)] + [next(hval) for _ in range(3)]
        state = np.random.get_state()
        np.random.seed(8)
        st, dm, dtrain, dval, dkt, dkv = D.dataloader(4, _args(ds, device_store='cpu'), maxlen=maxlen, frame_size=M.FRAME)
        assert isinstance(st, D.DeviceWordStore) and dm == hm and dkt == hkt and dkv == hkv and len(hkv) >= 1
        dev = [next(dtrain) for _ in range(3)] + [next(dval) for _ in range(3)]
        assert np.array_equal(state[1], np.random.get_state()[1])
        for h, d in zip(host, dev):
            assert h[:2] == d[:2] and isinstance(d[2], D.ClipBatch) and d[2].shape == h[2].shape
            assert np.array_equal(np.asarray(d[2]).view(np.int32), h[2].astype(np.float32).view(np.int32))
            _same_picks(h[3:], d[3:])
    # the store may stand in args.dataset, and the reference's pick_words reads it for a batch of words (loop.words_picker)
    np.random.seed(8)
    st2 = D.device_dataloader(4, _args(st), 'cpu', maxlen=M.MAXLEN, frame_size=M.FRAME)[0]
    assert st2 is st
    np.random.seed(3)
    a = D.pick_words(5, M.MAXLEN, ds, hkt, 7, None, frame_size=M.FRAME, skip_samples=True)
    np.random.seed(3)
    b = D.pick_words(5, M.MAXLEN, st, hkt, 7, None, frame_size=M.FRAME, skip_samples=True)
    _same_picks(a, b)
    # without device_store, and for the unconditional loader, nothing is routed
    assert not isinstance(D.dataloader(4, _args(ds), maxlen=M.MAXLEN)[0], D.DeviceWordStore)


def test_from_npz(monkeypatch, tmp_path):
    M.install(monkeypatch)
    path = os.path.join(tmp_path, 'w.npz')
    ingest.save_store(M.mapping(), path)
    st = D.DeviceWordStore.from_npz(path, 'cpu')
    assert torch.equal(st.bank.view(torch.int32), torch.from_numpy(M.pack(M.mapping())[0]).view(torch.int32))


def test_feeder_with_clips_gives_the_host_paths_static_tensors(monkeypatch):
    M.install(monkeypatch)
    from audiogan_amd import train
    ds, B, L = M.mapping(), 4, M.MAXLEN + M.FRAME          # (static rows wider than the loader's: zero-filled)
    np.random.seed(13)
    _, _, htrain, _, _, _ = D.dataloader(B, _args(ds), maxlen=M.MAXLEN, frame_size=M.FRAME)
    host = [train.batch_from_loader(next(htrain)) for _ in range(4)]
    np.random.seed(13)
    _, _, dtrain, _, _, _ = D.dataloader(B, _args(ds, device_store='cpu'), maxlen=M.MAXLEN, frame_size=M.FRAME)
    items = [next(dtrain) for _ in range(4)]
    mc = host[0]['cs'].shape[1]
    static = dict(real=torch.full((B, L), float('nan')), real_len=torch.zeros(B, dtype=torch.long),
                  cs=torch.zeros(B, mc, dtype=torch.long))
    f = train.Feeder(static, keys=['real', 'real_len', 'cs'], clips=('real', 'real_len'))
    assert f.keys == ['cs']
    seen = []

    class _G(object):
        def step(self):
            seen.append({k: v.clone() for k, v in static.items()})
    n = f.run(_G(), [dict(real=it[2], cs=np.asarray(it[5], dtype=np.int64)) for it in items])
    assert n == 4
    for h, s in zip(host, seen):
        want = np.zeros((B, L), np.float32)
        want[:, :M.MAXLEN] = h['real']
        assert np.array_equal(s['real'].numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(s['real_len'].numpy(), h['real_len']) and np.array_equal(s['cs'].numpy(), h['cs'])
    # batch_from_loader reads a ClipBatch as the float32 array it would have made itself
    assert np.array_equal(train.batch_from_loader(items[0])['real'], host[0]['real'])
    with pytest.raises(TypeError):
        f.stage(dict(real=host[0]['real'], cs=host[0]['cs']))
    with pytest.raises(ValueError):
        f.stage(dict(real=D.ClipBatch(items[0][2].store, [0, 1], M.MAXLEN), cs=host[0]['cs']))
    with pytest.raises(KeyError):
        train.Feeder(static, keys=['cs'], clips=('real', 'nope'))


def test_eager_loop_with_either_loader_on_the_kernel_model(monkeypatch):
    """TrainLoop._real gathers a ClipBatch into [B, L]: the same parameters, bit for bit, as from the host loader"""
    from tests import kernel_model
    kernel_model.install(monkeypatch)
    M.install(monkeypatch)
    import audiogan_amd as A
    (host, _), (dev, lp) = M.run_both_loaders(A, torch.device('cpu'), False, 4, 2)
    assert lp.dis_iter == 4 and lp.gen_iter == 2
    for p, q in zip(host, dev):
        assert torch.equal(p, q)


def test_refusals(store, monkeypatch):
    with pytest.raises(ValueError, match='clip ids'):
        D.ClipBatch(store, [0, store.n_clips], 8)
    with pytest.raises(ValueError, match='clip ids'):
        D.ClipBatch(store, [-1], 8)
    bad = M.mapping()
    bad['holes'] = bad['holes'].copy()
    bad['holes'][2, 5] = np.inf
    with pytest.raises(ValueError, match=r"clip 2 of word 'holes'"):
        D.DeviceWordStore(bad, 'cpu')
    bad['holes'][2, 5] = np.nan
    with pytest.raises(ValueError, match=r"clip 2 of word 'holes'"):
        D.DeviceWordStore(bad, 'cpu')
    empty = M.mapping()
    empty['void'] = np.zeros((0, 16), np.float32)
    with pytest.raises(ValueError, match="'void'"):
        D.DeviceWordStore(empty, 'cpu')
    # the model refuses what the wrapper refuses
    s = (store.bank, store.start, store.n_dev, store.peak)
    ids, out = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 8)
    with pytest.raises(TypeError):
        M.clip_gather(*s, ids.int(), out)
    with pytest.raises(TypeError):
        M.clip_gather(*s, ids, out.double())
    with pytest.raises(TypeError):
        M.clip_gather(*s, ids, out, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        M.clip_facts(store.bank, store.start.int(), store.cap)
    with pytest.raises(ValueError):
        M.clip_gather(*s, ids, torch.zeros(24).as_strided((3, 8), (4, 1)))


def test_launchers_refuse_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    import ctypes as C
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    buf = (C.c_char * 256)()
    p = C.addressof(buf) // 16 * 16 + 16

    def gather(**kw):
        a = dict(bank=p, start=p, n=p, peak=p, ids=p, B=2, out=p, ld=8, L=8, len_out=p, frame=0)
        a.update(kw)
        return K.lib.ag_clip_gather(a['bank'], a['start'], a['n'], a['peak'], a['ids'], a['B'], a['out'], a['ld'], a['L'],
                                    a['len_out'], a['frame'], None)
    for bad in (dict(ld=7), dict(B=-1), dict(B=65536), dict(L=-1), dict(frame=-1), dict(bank=p + 4), dict(bank=None),
                dict(ids=None), dict(out=None), dict(n=None), dict(peak=None), dict(start=None)):
        assert gather(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_clip_gather'), bad
    assert gather(B=0) == _lib.AG_OK and gather(B=0, bank=None, out=None) == _lib.AG_OK

    def facts(**kw):
        a = dict(bank=p, start=p, cap=p, n=p, peak=p, clips=3)
        a.update(kw)
        return K.lib.ag_clip_facts(a['bank'], a['start'], a['cap'], a['n'], a['peak'], a['clips'], None)
    for bad in (dict(clips=-1), dict(clips=1 << 31), dict(bank=p + 8), dict(bank=None), dict(cap=None), dict(peak=None)):
        assert facts(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_clip_facts'), bad
    assert facts(clips=0) == _lib.AG_OK and facts(clips=0, bank=None) == _lib.AG_OK
    assert K.lib.ag_abi_version() == 13
    header = open(os.path.join(ROOT, 'include', 'audiogan_hip.h')).read()
    for sym in ('ag_clip_facts', 'ag_clip_gather'):
        assert sym in _lib.SIGNATURES and 'int %s(' % sym in header

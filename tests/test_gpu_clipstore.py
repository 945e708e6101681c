"""The device-resident word store on the GPU (-m gpu): ag_clip_facts and ag_clip_gather under the checkers of
tests/clipstore_model.py (bit for bit against the host loader's rule, NaN-filled guarded destinations), a clip past 2^31 floats,
DeviceWordStore / pick_words / Feeder(clips=...) on a side stream, the eager and the captured TrainLoop and the Evaluator from
the host loader and from the device loader at the same seeds.  Every comparison is bit equality."""
import types

import numpy as np
import pytest
import torch

from audiogan_amd import dataset as D
from tests import clipstore_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


def _args(ds, **kw):
    return types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0, **kw)


def test_facts_on_the_table(K):
    """every clip of the table and the NaN / infinite clips: n and peak of the loader's rule, exact"""
    M.check_facts(K.clip_facts, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == 'clip_facts_kernel'


def test_gather_on_the_table(K):
    """widths 40, 41, 43, 1027 and one below a clip's n, a pitch beyond the width, out offset by one float, B 1 / 3 / 64,
    repeated ids: rows and lengths of the host loader bit for bit, nothing written outside a row's width"""
    seen = set()
    for case in M.gather_cases():
        M.run_gather(K.clip_gather, case, on=_cuda)
        seen.add(K.lib.ag_last_kernel().decode())
    assert seen == {'clip_gather_kernel<1>', 'clip_gather_kernel<0>'}          # 16-byte and scalar, both reached


def test_store_on_the_device_gathers_what_the_host_loader_picks(K):
    """DeviceWordStore on the GPU (a piece smaller than the bank: several uploads through the pinned buffer), its facts, and
    pick_words at the host function's seed"""
    ds = M.mapping()
    st = D.DeviceWordStore(ds, 'cuda', piece=512)
    bank = M.pack(ds)[0]
    assert st.bank.is_cuda and torch.equal(st.bank.cpu().view(torch.int32), torch.from_numpy(bank).view(torch.int32))
    M.run_gather(K.clip_gather, M.gather_cases()[0], on=_cuda, store=(st.bank, st.start, st.n_dev, st.peak))
    keys = list(ds)
    mc = max(len(k) for k in keys)
    np.random.seed(21)
    hk, hs, hl, hx, hn = D.pick_words(64, M.MAXLEN, ds, keys, mc, None, frame_size=M.FRAME)
    state = np.random.get_state()
    np.random.seed(21)
    dk, dsq, dl, batch, dn = st.pick_words(64, M.MAXLEN, keys, mc, frame_size=M.FRAME)
    assert np.array_equal(state[1], np.random.get_state()[1])
    assert np.array_equal(hk, dk) and np.array_equal(hs, dsq) and np.array_equal(hl, dl) and np.array_equal(hn, dn)
    assert np.array_equal(np.asarray(batch).view(np.int32), hx.astype(np.float32).view(np.int32))
    out, ln = batch.gather()
    assert out.is_cuda and tuple(out.shape) == (64, M.MAXLEN) and ln.tolist() == list(hn)
    bad = M.mapping()
    bad['tiny'] = bad['tiny'].copy()
    bad['tiny'][1, 0] = np.nan
    with pytest.raises(ValueError, match=r"clip 1 of word 'tiny'"):
        D.DeviceWordStore(bad, 'cuda')


def test_a_clip_past_2_to_31_floats(K):
    """64-bit starts: one clip at float 2^31 + 8 of an otherwise untouched bank (8.6 GB, never written or read elsewhere)"""
    rs = np.random.RandomState(5)
    far, cap = (1 << 31) + 8, 1101
    x = rs.uniform(-1, 1, cap).astype(np.float32)
    x[-1] = 0
    near = rs.uniform(-1, 1, 6).astype(np.float32)
    bank = torch.empty(far + 1104, dtype=torch.float32, device='cuda')
    bank[:8] = 0
    bank[:6] = torch.from_numpy(near).cuda()
    bank[far:] = 0
    bank[far:far + cap] = torch.from_numpy(x).cuda()
    start = torch.tensor([0, far], dtype=torch.int64).cuda()
    n, peak = K.clip_facts(bank, start, torch.tensor([6, cap], dtype=torch.int32).cuda())
    assert n.tolist() == [6, cap - 1]
    assert peak.cpu().numpy().view(np.int32).tolist() == [np.abs(near).max().view(np.int32), np.abs(x).max().view(np.int32)]
    flat = torch.full((3 * 1028 + 128,), float('nan')).cuda()
    out = flat[64:64 + 3 * 1028].view(3, 1028)[:, :1027]
    ln = torch.zeros(3, dtype=torch.int64).cuda()
    K.clip_gather(bank, start, n, peak, torch.tensor([1, 0, 1]).cuda(), out, ln, 200)
    rows = out.cpu().numpy()
    for b, clip in enumerate((x, near, x)):
        want, want_len = M.host_row(clip, 1027, 200)
        assert np.array_equal(rows[b].view(np.int32), want.view(np.int32)) and int(ln[b]) == want_len
    assert torch.isnan(flat[:64]).all() and torch.isnan(flat[64 + 3 * 1028:]).all()
    assert torch.isnan(flat[64:64 + 3 * 1028].view(3, 1028)[:, 1027:]).all()
    del bank
    torch.cuda.empty_cache()


def test_feeder_feeds_on_a_side_stream(K):
    """Feeder(clips=...): ids staged through their own pinned and device slots, the gather enqueued on the CURRENT stream"""
    from audiogan_amd import train
    ds, B, L = M.mapping(), 8, M.MAXLEN + M.FRAME
    np.random.seed(13)
    _, _, htrain, _, _, _ = D.dataloader(B, _args(ds), maxlen=M.MAXLEN, frame_size=M.FRAME)
    host = [train.batch_from_loader(next(htrain)) for _ in range(4)]
    np.random.seed(13)
    _, _, dtrain, _, _, _ = D.dataloader(B, _args(ds, device_store='cuda'), maxlen=M.MAXLEN, frame_size=M.FRAME)
    items = [next(dtrain) for _ in range(4)]
    static = dict(real=torch.full((B, L), float('nan')).cuda(), real_len=torch.zeros(B, dtype=torch.long).cuda(),
                  cs=torch.zeros(B, host[0]['cs'].shape[1], dtype=torch.long).cuda())
    f = train.Feeder(static, keys=['real', 'real_len', 'cs'], clips=('real', 'real_len'))
    assert f.keys == ['cs'] and f._ids_pin[0].is_pinned() and f._ids_dev[0].is_cuda
    seen = []

    class _G(object):
        def step(self):
            seen.append({k: v.clone() for k, v in static.items()})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        n = f.run(_G(), [dict(real=it[2], cs=np.asarray(it[5], dtype=np.int64)) for it in items])
    side.synchronize()
    assert n == 4
    for h, s in zip(host, seen):
        want = np.zeros((B, L), np.float32)
        want[:, :M.MAXLEN] = h['real']
        assert np.array_equal(s['real'].cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(s['real_len'].cpu().numpy(), h['real_len']) and np.array_equal(s['cs'].cpu().numpy(), h['cs'])


def test_eager_loop_from_either_loader(K):
    """at the widths tests/test_loop.py uses: two passes (4 critic + 2 generator iterations) from the host loader and from the
    device loader at the same seeds leave the same bits in every parameter"""
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    (host, _), (dev, lp) = M.run_both_loaders(A, torch.device('cuda'), True, 8, 2)
    assert lp.dis_iter == 4 and lp.gen_iter == 2 and K.lstm_persist_status() == 0
    for p, q in zip(host, dev):
        assert torch.equal(p, q)


def test_captured_loop_from_either_loader(K):
    """the captured loop (two eager warm-up passes, the captures, two replayed passes): the Feeder stages ids only and
    gathers into the static tensors; the same bits in every parameter as with the host loader"""
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    (host, lh), (dev, lp) = M.run_both_loaders(A, torch.device('cuda'), True, 8, 2, graphed=True)
    assert lp.dis_iter == 8 and lp.gen_iter == 4 and lp._graphs is not None and K.lstm_persist_status() == 0
    assert lp._feeder.clips == ('real', 'real_len') and lh._feeder.clips is None and 'real' not in lp._feeder.keys
    for p, q in zip(host, dev):
        assert torch.equal(p, q)


def test_evaluator_from_either_loader_holds_equal_tensors(K):
    """evaluate.Evaluator reads a ClipBatch as the array it would have cast itself"""
    import audiogan_amd as A
    from audiogan_amd import evaluate
    sets = []
    for device_store in (None, 'cuda'):
        _, (g, d, e_g, e_d), gen_val, ml = M.loop_setup(A, torch.device('cuda'), False, 4, device_store)
        ev = evaluate.Evaluator(g, d, e_g, e_d, gen_val, 4, ml, 'cuda', batches=2)
        sets.append(ev.set)
    assert len(sets[0]) == len(sets[1]) == 2
    for a, b in zip(*sets):
        assert sorted(a) == sorted(b)
        for k in ('real', 'real_len', 'cs', 'cl', 'z', 'u', 'real_power'):
            assert torch.equal(a[k], b[k]), k


def test_wrapper_refusals(K):
    st = D.DeviceWordStore(M.mapping(), 'cuda')
    s = (st.bank, st.start, st.n_dev, st.peak)
    ids, out = torch.zeros(3, dtype=torch.int64).cuda(), torch.zeros(3, 8).cuda()
    with pytest.raises(RuntimeError):
        K.clip_gather(*s, ids, out.cpu())
    with pytest.raises(TypeError):
        K.clip_gather(*s, ids.int(), out)
    with pytest.raises(TypeError):
        K.clip_gather(*s, ids, out.double())
    with pytest.raises(TypeError):
        K.clip_gather(*s, ids, out, torch.zeros(3, dtype=torch.int32).cuda())
    with pytest.raises(TypeError):
        K.clip_facts(st.bank, st.start.int(), st.cap)
    with pytest.raises(ValueError):
        K.clip_facts(st.bank[1:], st.start, st.cap)
    with pytest.raises(ValueError, match='pitch'):
        K.clip_gather(*s, ids, torch.zeros(24).cuda().as_strided((3, 8), (4, 1)))          # ld_out < L_out
    with pytest.raises(ValueError):
        K.clip_gather(*s, ids, torch.zeros(4, 8).cuda())
    with pytest.raises(ValueError, match='clip ids'):
        D.ClipBatch(st, [st.n_clips], 8)


def test_profiler_files_the_calls_under_the_reported_names(K):
    st = D.DeviceWordStore(M.mapping(), 'cuda')
    out = torch.empty(3, 40).cuda()
    K.Profiler.start()
    try:
        K.clip_facts(st.bank, st.start, st.cap)
        K.clip_gather(st.bank, st.start, st.n_dev, st.peak, torch.tensor([0, 1, 2]).cuda(), out)
    finally:
        rec = K.Profiler.stop()
    assert sorted(rec) == ['clip_facts_kernel', 'clip_gather_kernel<1>'] and all(r['n'] == 1 for r in rec.values())

"""Ingestion on the GPU (-m gpu): ag_resample_poly under the checkers of tests/ingest_model.py (the bound pass against float64,
the integer pass bit for bit, NaN-filled guarded destinations), chunks against the whole, out_start past 2^33, audio.resample and
ingest.build_store(device='cuda') on the CPU test's tree, the refused rate pair, the profiler.  The bounds: the module text of
tests/ingest_model.py; every ratio is printed before it is asserted."""
import os
import warnings

import numpy as np
import pytest
import torch

from audiogan_amd import audio, ingest
from tests import ingest_model
from tests.ingest_model import EXTRA_RATES, FAR_START, RATES, check_bound, check_bound_cases, check_integer, far_case, make_tree
from tests.test_ingest import check_store

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


@pytest.mark.parametrize('sr', RATES + EXTRA_RATES)
def test_bound_pass(K, sr):
    """both kinds x channels 1, 2, 3, three ragged rows (0, 1, half - 1 frames, 1023 / 1024 / 1025 / 2049 outputs), noise and a
    full-scale square wave, and the far case; 192 kHz: the launcher's smaller tile"""
    worst = check_bound(K.resample_poly, sr, on=_cuda)
    print('ag_resample_poly %d Hz: largest |y - y64| / bound %.4f' % (sr, worst))
    assert K.lib.ag_last_kernel().decode() == 'resample_poly_kernel'


@pytest.mark.parametrize('sr', RATES)
def test_integer_pass(K, sr):
    check_integer(K.resample_poly, sr, on=_cuda)


def test_the_largest_bank_takes_more_than_half_the_lds(K):
    """L = 1 with 16383 taps (65 532 bytes): window and bank of no tile fit 80 KB, so the launcher takes up to the CU's 160 KB.
    Integers, exact: the largest sum is 8 * 64 * 16383 < 2^24"""
    rs = np.random.RandomState(12)
    taps, n_in = 16383, 700
    bank = torch.from_numpy(rs.randint(-8, 9, size=(1, taps)).astype(np.float32))
    x = rs.randint(-64, 65, size=(2, n_in)).astype(np.float32)
    assert K.resample_ok(1, 1, taps, 1, 0)
    flat = torch.full((2 * 710 + 128,), float('nan')).cuda()
    dst = flat[64:64 + 2 * 710].view(2, 710)[:, :n_in]
    lens = torch.tensor([n_in, 333])
    y, counts = K.resample_poly(torch.from_numpy(x).cuda(), lens.cuda(), bank.cuda(), 1, 1, dst=dst)
    assert counts.tolist() == [700, 333] and torch.isnan(flat[:64]).all() and torch.isnan(flat[64 + 2 * 710:]).all()
    assert torch.isnan(flat[64:64 + 2 * 710].view(2, 710)[:, n_in:]).all()
    for b, n in enumerate(lens.tolist()):
        want = audio.resample_rule64(x[b, :n], bank.double().numpy(), 1, 1, n_out=n_in)
        assert np.abs(want).max() < 2 ** 24 and np.array_equal(y[b].cpu().double().numpy(), want), b


def test_chunks_have_the_bits_of_the_whole(K):
    """a 44.1 kHz row of 40 000 frames at once and in chunks of 1000 outputs, each chunk a row of its own holding the frames its
    outputs read (half either side), with in_start / out_start"""
    rs = np.random.RandomState(4)
    L, M, half, bank = audio.resample_bank(44100, device='cuda')
    for C, dt in ((1, np.float32), (2, np.int16)):
        x = (rs.uniform(-1, 1, (1, 40000, C)) * (30000 if dt is np.int16 else 1)).astype(dt)
        xs = torch.from_numpy(x).cuda()
        whole, counts = K.resample_poly(xs if C > 1 else xs[:, :, 0], None, bank, L, M)
        n_out = audio.out_count(40000, L, M)
        assert tuple(whole.shape) == (1, n_out) and counts.tolist() == [n_out]
        parts = torch.full_like(whole, float('nan'))
        for o0 in range(0, n_out, 1000):
            o1 = min(n_out, o0 + 1000)
            lo, hi = max(0, (o0 * M) // L - half), min(40000, ((o1 - 1) * M) // L + half + 1)
            row = xs[:, lo:hi].contiguous()
            K.resample_poly(row if C > 1 else row[:, :, 0], None, bank, L, M, dst=parts[:, o0:o1], in_start=lo, out_start=o0)
        assert torch.equal(whole.view(torch.int32), parts.view(torch.int32)), C
        # and through audio.resample, which uploads a host source window by window
        y_all, c_all = audio.resample(x, 44100, device='cuda')
        y_chk, c_chk = audio.resample(x, 44100, device='cuda', chunk=1000)
        assert y_all.is_cuda and torch.equal(y_all, whole) and torch.equal(y_chk, whole)
        assert c_all.tolist() == c_chk.tolist() == [n_out]


def test_out_start_past_2_to_33(K):
    """one small launch at out_start = 2^33 against the float64 rule evaluated with Python integers: N M passes 2^41"""
    case = far_case(44100)
    assert case['out_start'] == FAR_START and (FAR_START * 441) > (1 << 41) and case['in_start'] > (1 << 35)
    check_bound_cases(K.resample_poly, [case], on=_cuda)
    check_bound_cases(K.resample_poly, [far_case(11025), far_case(48000)], on=_cuda)


def test_wrapper_bad_arguments(K):
    L, M, half, bank = audio.resample_bank(16000, device='cuda')
    x = torch.zeros(2, 100, device='cuda')
    with pytest.raises(RuntimeError):
        K.resample_poly(x.cpu(), None, bank, L, M)
    with pytest.raises(TypeError):
        K.resample_poly(x.double(), None, bank, L, M)
    with pytest.raises(TypeError):
        K.resample_poly(x, torch.zeros(2, dtype=torch.int32, device='cuda'), bank, L, M)
    with pytest.raises(ValueError):
        K.resample_poly(x, None, bank[:, :68].contiguous(), L, M)
    y, counts = K.resample_poly(x, None, bank, L, M, n_out=0)
    assert tuple(y.shape) == (2, 0) and counts.tolist() == [50, 50]
    assert audio.resample_bank(16000, device='cuda')[3] is bank and bank.is_cuda


def test_resample_and_build_store_on_the_device(K, tmp_path):
    """the CPU test's tree through build_store(device='cuda'): the words, counts and shapes of the float64 path, every sample
    within the bound of the launch; a refused rate pair takes the host path with its warning"""
    entries, facts = make_tree(os.path.join(tmp_path, 'tree'))
    store, report = ingest.build_store(entries, maxlen=ingest_model.TREE_MAXLEN, device='cuda')
    check_store(store, report, facts, exact=False)
    host, _ = ingest.build_store(entries, maxlen=ingest_model.TREE_MAXLEN, device='cpu')
    assert list(host) == list(store) and all(host[w].shape == store[w].shape for w in host)
    cut = dict(alpha=[('a1', slice(None)), ('a2', slice(None))], beta=[('b1', slice(None))],
               delta=[('a1', slice(400, 1600)), ('a1', slice(2000, 3600))])
    worst = 0.0
    for w, clips in cut.items():
        for i, (name, sl) in enumerate(clips):
            x, sr = facts['sources'][name]
            L, M, half, bank = audio.resample_bank(sr)
            C = x.shape[1] if x.ndim == 2 else 1
            x64 = x.astype(np.float64).reshape(len(x), C).sum(1) / C * (2.0 ** -15 if x.dtype == np.int16 else 1.0)
            b64 = bank.double().numpy()
            y64 = audio.resample_rule64(x64, b64, L, M)[sl]
            s = audio.resample_rule64(np.abs(x64), np.abs(b64), L, M)[sl]
            got = store[w][i, :len(y64)].astype(np.float64)
            ratio = float((np.abs(got - y64) / ((bank.size(1) + C + 3) * 2.0 ** -24 * s + 1e-30)).max())
            worst = max(worst, ratio)
            print('build_store on the device, %s[%d]: |y - y64| / bound %.4f' % (w, i, ratio))
            assert ratio <= 1.0, (w, i, ratio)
    # ragged rows: zero at and past a row's count, as on the host path
    xr = np.random.RandomState(2).randint(-3000, 3000, size=(2, 900, 2)).astype(np.int16)
    yr, cr = audio.resample(xr, 44100, lens=[900, 441], device='cuda')
    assert yr.is_cuda and tuple(yr.shape) == (2, 164) and cr.tolist() == [164, 80]
    assert not yr[1, 80:].any() and yr[1, :80].any() and yr[0, 163] != 0
    x = np.random.RandomState(9).uniform(-1, 1, 500).astype(np.float32)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        y, counts = audio.resample(x, 44099, device='cuda')
    assert len([w for w in seen if '44099 -> 8000' in str(w.message)]) == 1, [str(w.message) for w in seen]
    assert y.is_cuda and counts.tolist() == [91]
    assert np.array_equal(y.cpu().numpy()[0], audio.resample64(x, 44099).astype(np.float32))


def test_profiler_files_the_call_under_the_reported_name(K):
    L, M, half, bank = audio.resample_bank(44100, device='cuda')
    x = torch.zeros(2, 5000, 2, dtype=torch.int16, device='cuda')
    K.Profiler.start()
    try:
        K.resample_poly(x, None, bank, L, M)
    finally:
        rec = K.Profiler.stop()
    assert list(rec) == ['resample_poly_kernel'] and rec['resample_poly_kernel']['n'] == 1
    assert K.lib.ag_last_kernel().decode() == 'resample_poly_kernel'

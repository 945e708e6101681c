"""Ingestion on the CPU: audio.read_wav, audio.resample_bank / resample64 (the filter facts), the model of ag_resample_poly
(tests/ingest_model.py) under the GPU checkers and the mutants they must reject, the launcher's refusals (host code, no GPU),
ingest.build_store / save_store / load_store, the loader on the .npz and the command-line tool.  -m gpu: tests/test_gpu_ingest.py.

The bounds and where they come from: the module text of tests/ingest_model.py."""
import argparse
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from audiogan_amd import audio, dataset, ingest
from tests import ingest_model
from tests.ingest_model import MUTANTS, RATES, check_bound, check_integer, make_tree, pcm16, wav_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {44100: (80, 441, 187), 48000: (1, 6, 205), 22050: (160, 441, 95), 16000: (1, 2, 69), 11025: (320, 441, 49),
          6000: (4, 3, 35), 4000: (2, 1, 35)}


# ------------------------------------------------------------------------------------------------------------------
# 1. the bank
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', sorted(SHAPES))
def test_bank_facts_and_tones(sr):
    L, M, half, bank = audio.resample_bank(sr)
    assert (L, M, 2 * half + 1) == SHAPES[sr] and tuple(bank.shape) == (L, SHAPES[sr][2]) and bank.dtype == torch.float32
    assert audio.resample_bank(sr)[3] is bank          # cached
    b = bank.double().numpy()
    assert np.abs(b.sum(1) - 1.0).max() <= 1e-4 and np.abs(b).sum(1).max() <= 2.21
    n = sr // 2
    t_in = np.arange(n) / float(sr)
    top = {4000: 1450.0, 6000: 1750.0}.get(sr, 2950.0)          # (a 6 kHz input's own band ends at 0.95 x 3000 Hz)
    for f in (300.0, 1000.0, top):
        y = audio.resample64(np.sin(2 * np.pi * f * t_in).astype(np.float32), sr)
        assert y.dtype == np.float64 and y.shape == (audio.out_count(n, L, M),)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / 8000.0)
        err = 10 * np.log10(((y - want)[200:-200] ** 2).mean() / 0.5)
        print('%d Hz -> 8000 Hz, tone %g Hz: %.1f dB' % (sr, f, err))
        assert err <= -80.0, (sr, f, err)
    for f in (4400.0, 5000.0, 7000.0):
        if f < sr / 2.0:
            y = audio.resample64(np.sin(2 * np.pi * f * t_in).astype(np.float32), sr)
            res = 10 * np.log10((y[200:-200] ** 2).mean() / 0.5)
            print('%d Hz -> 8000 Hz, tone %g Hz: residual %.1f dB' % (sr, f, res))
            assert res <= -70.0, (sr, f, res)


def test_equal_rates_return_the_input():
    x = np.random.RandomState(0).uniform(-1, 1, 1000).astype(np.float32)
    assert np.array_equal(audio.resample64(x, 8000), x.astype(np.float64))
    y, counts = audio.resample(x, 8000, device='cpu')
    assert y.dtype == torch.float32 and np.array_equal(y.numpy()[0], x) and counts.tolist() == [1000]
    x16 = (x * 30000).astype(np.int16)
    assert np.array_equal(audio.resample(x16, 8000, device='cpu')[0].numpy()[0], x16.astype(np.float32) * np.float32(2.0 ** -15))


# ------------------------------------------------------------------------------------------------------------------
# 2. read_wav
# ------------------------------------------------------------------------------------------------------------------
def _put(tmp_path, name, blob):
    path = os.path.join(tmp_path, name)
    with open(path, 'wb') as f:
        f.write(blob)
    return path


def _pcm24(v):
    return b''.join(struct.pack('<i', int(s))[:3] for s in v)


@pytest.mark.parametrize('channels', (1, 2))
def test_read_wav_formats(tmp_path, channels):
    rs = np.random.RandomState(channels)
    n = 37 * channels
    v8 = rs.randint(0, 256, n)
    v16 = np.concatenate([[-32768, 32767, 0, -1][:n], rs.randint(-32768, 32768, n - 4)])
    v24 = np.concatenate([[-(1 << 23), (1 << 23) - 1, 0, -1], rs.randint(-(1 << 23), 1 << 23, n - 4)])
    v32 = np.concatenate([[-(1 << 31), (1 << 31) - 1, 0, -1], rs.randint(-(1 << 31), 1 << 31, n - 4)])
    f = rs.uniform(-2, 2, n)
    table = [
        (wav_bytes(v8.astype('u1').tobytes(), 8000, channels, 8), ((v8 - 128.0) / 128.0).astype(np.float32), 8000),
        (wav_bytes(pcm16(v16), 16000, channels, 16), v16.astype(np.int16), 16000),
        (wav_bytes(_pcm24(v24), 44100, channels, 24), (v24 / float(1 << 23)).astype(np.float32), 44100),
        (wav_bytes(v32.astype('<i4').tobytes(), 48000, channels, 32), (v32 / float(1 << 31)).astype(np.float32), 48000),
        (wav_bytes(f.astype('<f4').tobytes(), 22050, channels, 32, tag=3), f.astype(np.float32), 22050),
        (wav_bytes(f.astype('<f8').tobytes(), 11025, channels, 64, tag=3), f.astype(np.float32), 11025),
        (wav_bytes(pcm16(v16), 16000, channels, 16, extensible=True), v16.astype(np.int16), 16000),
        (wav_bytes(f.astype('<f4').tobytes(), 8000, channels, 32, tag=3, extensible=True), f.astype(np.float32), 8000),
    ]
    for i, (blob, want, sr) in enumerate(table):
        data, got_sr = audio.read_wav(_put(tmp_path, 'f%d.wav' % i, blob))
        assert got_sr == sr and data.dtype == want.dtype and data.shape == (37, channels), i
        assert np.array_equal(data, want.reshape(37, channels)), i


def test_read_wav_chunks_sizes_and_truncation(tmp_path):
    v = np.arange(-50, 50).astype(np.int16)
    pay = pcm16(v)
    # an unknown chunk before data; an odd-sized chunk with its pad byte
    blob = wav_bytes(pay, 16000, 2, 16, before=b'LIST' + struct.pack('<I', 4) + b'abcd' + b'junk' + struct.pack('<I', 3) +
                     b'xyz' + b'\x00')
    data, sr = audio.read_wav(_put(tmp_path, 'chunks.wav', blob))
    assert sr == 16000 and np.array_equal(data, v.reshape(50, 2))
    # (without honouring the pad byte the reader would look for a chunk id one byte early and find no data)
    for size in (0xFFFFFFFF, 0):
        data, _ = audio.read_wav(_put(tmp_path, 'open.wav', wav_bytes(pay, 16000, 2, 16, data_size=size)))
        assert np.array_equal(data, v.reshape(50, 2)), size
    # cut in the middle of a frame: the whole frames
    data, _ = audio.read_wav(_put(tmp_path, 'cut.wav', wav_bytes(pay, 16000, 2, 16)[:-5]))
    assert np.array_equal(data, v.reshape(50, 2)[:48])
    # data followed by another chunk: the size is honoured
    data, _ = audio.read_wav(_put(tmp_path, 'tail.wav', wav_bytes(pay, 16000, 1, 16) + b'LIST' + struct.pack('<I', 2) + b'ab'))
    assert np.array_equal(data, v.reshape(100, 1))


def test_read_wav_refusals(tmp_path):
    pay = pcm16(np.arange(8))
    good = wav_bytes(pay, 8000, 1, 16)
    no_fmt = b'RIFF' + struct.pack('<I', 4 + 8 + len(pay)) + b'WAVE' + b'data' + struct.pack('<I', len(pay)) + pay
    table = [
        (wav_bytes(pay, 8000, 1, 16, riff=b'RIFX'), 'RIFF/WAVE'),
        (wav_bytes(pay, 8000, 1, 16, wave=b'AVI '), 'RIFF/WAVE'),
        (b'RIF', 'RIFF/WAVE'),
        (no_fmt, 'no fmt chunk before data'),
        (wav_bytes(pay, 8000, 1, 4, tag=0x11), 'compressed'),
        (wav_bytes(pay, 8000, 1, 16, tag=0x55, extensible=True), 'compressed'),
        (wav_bytes(pay, 8000, 0, 16), 'zero channels'),
        (wav_bytes(pay, 8000, 1, 12), '12 bits'),
        (good[:36], 'no data chunk'),
    ]
    for i, (blob, why) in enumerate(table):
        path = _put(tmp_path, 'bad%d.wav' % i, blob)
        with pytest.raises(ValueError) as e:
            audio.read_wav(path)
        assert path in str(e.value) and why in str(e.value), (i, str(e.value))


def test_write_wav_round_trip(tmp_path):
    x = np.random.RandomState(3).randn(1234).astype(np.float32)
    x[:4] = [0.0, -0.0, np.float32(1e-40), np.float32(3e38)]
    path = os.path.join(tmp_path, 'rt.wav')
    audio.write_wav(path, x, sr=8000)
    data, sr = audio.read_wav(path)
    assert sr == 8000 and data.dtype == np.float32 and data.shape == (1234, 1)
    assert np.array_equal(data[:, 0].view(np.int32), x.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------
# 3. the model under the GPU checkers; the mutants
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', RATES)
def test_model_against_float64(sr):
    worst = check_bound(ingest_model.resample_poly, sr)
    print('model, %d Hz: largest |y - y64| / bound %.4f' % (sr, worst))
    check_integer(ingest_model.resample_poly, sr)


@pytest.mark.parametrize('mutant', MUTANTS)
def test_checkers_reject_mutants(mutant):
    """phase (N M) mod M, base off by one, the window not centred, N M in 32 bits, a frame at or past len_b read, int16 scaled
    by 1 / 32767, channels not averaged: the integer pass and the bound pass must both fail (at 44.1 kHz: L > 1, 187 taps)"""
    fn = lambda *a, **k: ingest_model.resample_poly(*a, mutate=mutant, **k)          # noqa: E731
    with pytest.raises(AssertionError):
        check_integer(fn, 44100)
    with pytest.raises(AssertionError):
        check_bound(fn, 44100)


# ------------------------------------------------------------------------------------------------------------------
# 4. the launcher
# ------------------------------------------------------------------------------------------------------------------
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15


def test_launcher_refuses_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    p = ctypes.c_void_p(PTR)
    ok = dict(src=p, kind=1, C=2, pitch=2000, lens=p, n_in=1000, in_start=0, bank=p, L=80, M=441, taps=187, dst=p, ldd=200,
              n_out=182, out_start=0, B=3)

    def call(**kw):
        a = dict(ok, **kw)
        return K.lib.ag_resample_poly(a['src'], a['kind'], a['C'], a['pitch'], a['lens'], a['n_in'], a['in_start'], a['bank'],
                                      a['L'], a['M'], a['taps'], a['dst'], a['ldd'], a['n_out'], a['out_start'], a['B'], None)
    for bad in (dict(L=88), dict(L=322, taps=51), dict(taps=186), dict(taps=1), dict(C=0), dict(C=9), dict(kind=2), dict(kind=-1),
                dict(M=(1 << 20) + 1), dict(n_in=-1), dict(n_out=-1), dict(B=-1), dict(pitch=-1), dict(ldd=-1),
                dict(src=None), dict(dst=None), dict(bank=None), dict(pitch=1999), dict(ldd=181)):
        assert call(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_resample_poly'), bad
    assert call(B=0) == _lib.AG_OK and call(n_out=0) == _lib.AG_OK
    assert call(B=0, src=None, dst=None, bank=None) == _lib.AG_OK
    for args, want in (((80, 441, 187, 1, 0), 1), ((320, 441, 49, 8, 1), 1), ((1, 6, 205, 3, 1), 1), ((1, 1, 16383, 1, 0), 1),
                       ((1, 1, 16385, 1, 0), 0), ((8000, 44099, 187, 1, 0), 0), ((80, 441, 188, 1, 0), 0), ((1, 2, 1, 1, 0), 0),
                       ((1, 2, 69, 0, 0), 0), ((1, 2, 69, 9, 0), 0), ((1, 2, 69, 1, 2), 0)):
        assert K.lib.ag_resample_ok(*args) == want, args
        assert ingest_model.resample_ok(*args) == bool(want) and K.resample_ok(*args) == bool(want), args
    assert K.lib.ag_abi_version() == 13
    header = open(os.path.join(ROOT, 'include', 'audiogan_hip.h')).read()
    for sym in ('ag_resample_ok', 'ag_resample_poly'):
        assert sym in _lib.SIGNATURES and 'int %s(' % sym in header
    assert 'preprocess.py:24' in header and 'preprocess-fisher.py:232' in header


# ------------------------------------------------------------------------------------------------------------------
# 5. build_store, the store on disk, the loader
# ------------------------------------------------------------------------------------------------------------------
def check_store(store, report, facts, exact):
    """words, clip counts, shapes and the report; ``exact``: the float64 path's bits"""
    want = facts['want']
    assert type(store) is dict and list(store) == ['alpha', 'beta', 'delta']
    assert report['kept'] == dict(alpha=2, beta=1, delta=2)
    p = facts['paths']
    assert report['dropped'] == dict(silent=[p['silent']], too_long=[p['long']], unreadable=[p['broken']])
    assert abs(report['seconds_in'] - (0.5 + 0.4 + 0.3 + 0.25 + 1.2)) < 1e-9
    for w, clips in want.items():
        lens = [ingest.clip_length(c) for c in clips]
        assert store[w].dtype == np.float32 and store[w].shape == (len(clips), max(lens)), (w, store[w].shape)
        for i, (c, n) in enumerate(zip(clips, lens)):
            assert not store[w][i, n:].any()
            if exact:
                assert np.array_equal(store[w][i, :n], c[:n]), (w, i)
    assert abs(report['seconds_out'] - sum(ingest.clip_length(c) for cs in want.values() for c in cs) / 8000.0) < 1e-9


def test_build_store_save_load_and_loader(tmp_path):
    entries, facts = make_tree(os.path.join(tmp_path, 'tree'))
    assert [e[1] for e in entries] == ['alpha', 'alpha', 'beta', 'beta', 'gamma', 'gamma', 'delta', 'delta']
    assert entries[-2] == (facts['paths']['a1'], 'delta', 0.05, 0.2) and entries[0] == (facts['paths']['a1'], 'alpha', None, None)
    out = os.path.join(tmp_path, 'words.npz')
    store, report = ingest.build_store(entries, out_path=out, maxlen=ingest_model.TREE_MAXLEN, device='cpu')
    check_store(store, report, facts, exact=True)
    assert store['alpha'].shape == (2, 4000) and store['beta'].shape == (1, 2400) and store['delta'].shape == (2, 1600)
    loaded = ingest.load_store(out)
    assert type(loaded) is dict and list(loaded) == list(store)
    assert all(loaded[w].dtype == np.float32 and np.array_equal(loaded[w].view(np.int32), store[w].view(np.int32)) for w in store)
    odd = {'a/b': store['alpha'], '..': store['beta'], u'café ☃': store['delta'], '': store['beta']}
    ingest.save_store(odd, out)
    back = ingest.load_store(out)
    assert list(back) == list(odd) and all(np.array_equal(back[w], odd[w]) for w in odd)
    ingest.save_store(store, out)
    # the loader: the path and the loaded mapping give the same minibatch under the same numpy seed
    got = []
    for spec in (out, loaded):
        args = argparse.Namespace(dataset=spec, conditional=True, minwordlen=1)
        np.random.seed(5)
        ds, maxlen, gen_train, gen_val, keys_train, keys_val = dataset.dataloader(4, args, frame_size=200)
        assert type(ds) is dict and maxlen == 4000 and sorted(keys_train + keys_val) == ['alpha', 'beta', 'delta']
        got.append(next(gen_val))
    for a, b in zip(*got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    _, _, samples, lengths, picked, cseq, clen = got[0]
    assert samples.shape == (4, 4000) and all(k in store for k in picked)
    for b in range(4):
        assert np.abs(samples[b]).max() == 1.0 and lengths[b] % 200 == 0 and 0 < lengths[b] <= 4000
        assert not samples[b, lengths[b]:].any()


def test_open_takes_an_npz_without_h5py(tmp_path):
    path = os.path.join(tmp_path, 's.npz')
    ingest.save_store({'word': np.ones((2, 5), dtype=np.float32)}, path)
    assert dataset._open(path)['word'].shape == (2, 5)
    spec = {'data': np.zeros((3, 4))}
    assert dataset._open(spec) is spec


def test_manifest_rules(tmp_path):
    tsv = os.path.join(tmp_path, 'm.tsv')
    with open(tsv, 'w') as f:
        f.write('# head\n\nx.wav\tone\n/abs/y.wav\ttwo\t1.5\t2\n')
    assert ingest.read_manifest(tsv) == [(os.path.join(str(tmp_path), 'x.wav'), 'one', None, None),
                                         ('/abs/y.wav', 'two', 1.5, 2.0)]
    with open(tsv, 'w') as f:
        f.write('x.wav\tone\t1.0\n')
    with pytest.raises(ValueError):
        ingest.read_manifest(tsv)


def test_resample_rows_on_the_host():
    """[n], [B, n] and [B, n, C] with ragged lengths: the float64 path, zero past the counts"""
    rs = np.random.RandomState(2)
    x = rs.randint(-3000, 3000, size=(2, 900, 2)).astype(np.int16)
    y, counts = audio.resample(x, 44100, lens=[900, 441], device='cpu')
    assert tuple(y.shape) == (2, 164) and counts.tolist() == [164, 80] and not y[1, 80:].any()
    assert np.array_equal(y[1, :80].numpy(), audio.resample64(x[1, :441], 44100).astype(np.float32))
    y1, c1 = audio.resample(torch.from_numpy(x[0, :, 0].copy()), 44100, device='cpu')
    assert tuple(y1.shape) == (1, 164) and np.array_equal(y1[0].numpy(), audio.resample64(x[0, :, 0], 44100).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------
# 6. the command-line tool
# ------------------------------------------------------------------------------------------------------------------
def _tool(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', 'audiogan_amd.ingest'] + list(argv), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True)


def test_command_line_tool(tmp_path, capsys):
    root = os.path.join(tmp_path, 'tree')
    _, facts = make_tree(root)
    out = os.path.join(tmp_path, 'cli.npz')
    r = _tool('--tree', root, '--out', out, '--maxlen', str(ingest_model.TREE_MAXLEN), '--device', 'cpu')
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep['kept'] == dict(alpha=2, beta=1) and rep['dropped'] == dict(silent=1, too_long=1, unreadable=1)
    assert abs(rep['seconds_in'] - 2.65) < 1e-9 and abs(rep['seconds_out'] - (4000 + 3200 + 2400) / 8000.0) < 1e-9
    assert sorted(ingest.load_store(out)) == ['alpha', 'beta']
    # (the manifest form in this process: the exit status of a process is checked above and below)
    assert ingest.main(['--manifest', facts['tsv'], '--out', out, '--device', 'cpu']) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['kept'] == dict(delta=2)
    assert sorted(ingest.load_store(out)) == ['delta']
    empty = os.path.join(tmp_path, 'empty')
    os.makedirs(os.path.join(empty, 'word'))
    none = os.path.join(tmp_path, 'none.npz')
    r = _tool('--tree', empty, '--out', none)
    assert r.returncode != 0 and json.loads(r.stdout.strip().splitlines()[-1])['kept'] == {} and not os.path.exists(none)

"""Generator.generate (sampling with the stop draws and the early exit of the frame loop), the TrainLoop sampling hook and
audio.write_wav - host logic on CPU, the HIP kernels replaced by the torch model of tests/kernel_model.py.  The generation
launch itself (ag_gfront_fwd, gen = 1) is modelled here (``gfront_gen_persist``): the persistent host path runs on it when
``gfront_persist_ok`` is patched to True.  The real launch is covered by tests/test_gpu_generate.py (-m gpu)."""
import os
import struct

import numpy as np
import pytest
import torch

from oracle import audiogan_oracle as O
from tests import kernel_model

GEN_LAG = 1      # csrc/front_parts.h: the exit test before frame t + 1 reads the decisions of frame t - GEN_LAG


def gfront_gen_persist(pre, wx, whh, wp, bp, ws, bs, u, x, s, first, t_run, bhn=None):
    """torch model of ag_gfront_fwd in generation mode (include/audiogan_hip.h): the frame loop with the stop draws and the exit rule"""
    T, B, SG = pre.shape
    S, fs = whh.size(1), wp.size(0)
    gru = SG == 3 * S
    h, c, xp = torch.zeros(B, S), torch.zeros(B, S), torch.zeros(B, fs)
    fst = torch.full((B,), T, dtype=torch.int32)
    ran = T
    for t in range(T):
        if t > GEN_LAG and bool((fst <= t - GEN_LAG).all()):
            ran = t
            break
        if gru:
            gi, gh = pre[t] + xp @ wx.t(), h @ whh.t()
            r, z = torch.sigmoid(gi[:, :S] + gh[:, :S]), torch.sigmoid(gi[:, S:2 * S] + gh[:, S:2 * S])
            n = torch.tanh(gi[:, 2 * S:] + r * (gh[:, 2 * S:] + bhn))
            h = (1 - z) * n + z * h
        else:
            g = pre[t] + xp @ wx.t() + h @ whh.t()
            i, f, gg, o = g.chunk(4, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
        xp = torch.tanh(h @ wp.t() + bp)
        x[:, t * fs:(t + 1) * fs] = xp
        sv = h @ ws.view(-1) + bs
        s[:, t] = sv
        fst[(fst == T) & (u[t] < torch.sigmoid(sv))] = t + 1
    first.copy_(fst)
    t_run.fill_(ran)


@pytest.fixture(autouse=True)
def _model_kernels(monkeypatch):
    kernel_model.install(monkeypatch)
    import audiogan_amd.kernels as K
    monkeypatch.setattr(K, 'gfront_gen_persist', gfront_gen_persist)


def _persist(monkeypatch, on):
    """on: the persistent host path (the modelled generation launch); off: the per-frame fallback"""
    import audiogan_amd.kernels as K
    monkeypatch.setattr(K, 'gfront_persist_ok', lambda B, S, fs, dev: bool(on))


GCFG = dict(frame_size=32, embed_size=8, noise_size=8, state_size=64, struct=[[17, 8, 16, 8], [9, 4, 16, 8]])


def _pair(gru):
    import audiogan_amd as A
    torch.manual_seed(11)
    if gru:
        go = O.GRUGenerator(**GCFG)
        g = A.GRUGenerator(**GCFG)
    else:
        go = O.Generator(num_layers=1, **GCFG)
        g = A.Generator(num_layers=1, **GCFG)
    g.load_state_dict(go.state_dict())
    return g, go


def _u_stops_at(frames, T):
    """u [T,B]: 0 at clip b's stop frame (always a stop), 1 elsewhere (never a stop); frame None = the clip never stops"""
    u = torch.ones(T, len(frames))
    for b, k in enumerate(frames):
        if k is not None:
            u[k, b] = 0.0
    return u


def _close(got, ref, rtol=1e-4, atol=1e-5, msg=''):
    np.testing.assert_allclose(got.detach().numpy(), ref.detach().numpy(), rtol=rtol, atol=atol, err_msg=msg)


def _check_draws(u, s, stop_list):
    """the returned decisions are u < sigmoid(s) recomputed from the returned logits, wherever that is not a tie"""
    t_eff = s.size(1)
    draws = torch.cat(stop_list, 1)
    assert tuple(draws.shape) == tuple(s.shape)
    p, uu = torch.sigmoid(s), u[:t_eff].t()
    clear = (uu - p).abs() > 1e-5
    assert torch.equal(draws.bool()[clear], (uu < p)[clear])
    return draws


@pytest.mark.parametrize('persist', [False, True])
def test_generate_vs_oracle_deterministic_stops(monkeypatch, persist):
    _persist(monkeypatch, persist)
    g, go = _pair(False)
    B, T, fs = 5, 6, 32
    gen = torch.Generator().manual_seed(3)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    for frames in ([2, 0, 4, None, 1], [2, 0, 3, 1, 1]):      # one clip never stops / every clip stops by frame 3
        u = _u_stops_at(frames, T)
        wave, s, stop_list, length = g.generate(c, z=z, u=u)
        want = torch.tensor([T if k is None else k + 1 for k in frames])
        assert torch.equal(length, want * fs)
        t_eff = int(want.max())
        assert len(stop_list) == t_eff and tuple(s.shape) == (B, t_eff) and tuple(wave.shape) == (B, t_eff * fs)
        assert not wave.requires_grad and not s.requires_grad
        if persist:
            assert int(g.last_t_run) == min(T, t_eff + GEN_LAG)
        else:
            assert g.last_t_run is None
        stops = _check_draws(u, s, stop_list)
        wo, so, _, lo = go(z=z, c=c, stop=stops)
        assert torch.equal(length, lo)
        _close(wave, wo, msg='wave')
        _close(s, so, msg='stop logits')


@pytest.mark.parametrize('persist', [False, True])
def test_generate_vs_oracle_random_stops(monkeypatch, persist):
    _persist(monkeypatch, persist)
    g, go = _pair(False)
    B, T, fs = 6, 8, 32
    gen = torch.Generator().manual_seed(5)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    wave, s, stop_list, length = g.generate(c, z=z, generator=torch.Generator().manual_seed(9))
    u = torch.rand(T, B, generator=torch.Generator().manual_seed(9))     # what a seeded generator reproduces
    stops = _check_draws(u, s, stop_list)
    from audiogan_amd.recurrent import first_stops
    assert torch.equal(length, first_stops(stops, T) * fs)
    wo, so, _, lo = go(z=z, c=c, stop=stops)
    assert torch.equal(length, lo)
    _close(wave, wo, msg='wave')
    _close(s, so, msg='stop logits')
    w2, s2, _, l2 = g.generate(c, z=z, u=u)
    assert torch.equal(w2, wave) and torch.equal(s2, s) and torch.equal(l2, length)


@pytest.mark.parametrize('persist', [False, True])
def test_gru_generate_vs_oracle(monkeypatch, persist):
    """GRUGenerator (BASELINE C4): the oracle has no stop draws, so it runs on the first t_eff frames of z (the frames depend
    on the past only) and its logits decide the draws"""
    _persist(monkeypatch, persist)
    g, go = _pair(True)
    B, T, fs = 5, 6, 32
    gen = torch.Generator().manual_seed(13)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    for u in (_u_stops_at([1, 3, None, 0, 2], T), _u_stops_at([1, 3, 2, 0, 2], T), torch.rand(T, B, generator=gen)):
        wave, s, stop_list, length = g.generate(c, z=z, u=u)
        t_eff = s.size(1)
        stops = _check_draws(u, s, stop_list)
        from audiogan_amd.recurrent import first_stops
        assert torch.equal(length, first_stops(stops, T) * fs) and int(length.max()) == t_eff * fs
        wo, so, _, _ = go(z=z[:, :t_eff], c=c)
        _close(wave, wo, msg='wave')
        _close(s, so, msg='stop logits')


def test_generate_uses_current_weights_after_raw_writes(monkeypatch):
    """a captured optimiser step rewrites the parameters through raw pointers (no version bump): generate must not sample
    with the weights materialised before"""
    _persist(monkeypatch, True)
    g, go = _pair(False)
    B, T = 3, 5
    gen = torch.Generator().manual_seed(17)
    z, c = torch.randn(B, T, 8, generator=gen), torch.randn(B, 8, generator=gen)
    u = _u_stops_at([1, 4, 2], T)
    g.generate(c, z=z, u=u)
    with torch.no_grad():
        for p_ in list(g.parameters()):
            p_.data.mul_(1.1)           # (.data: like a raw-pointer write, the version seen through the Parameter is unchanged)
        for p_ in list(go.parameters()):
            p_.mul_(1.1)
    wave, s, stop_list, length = g.generate(c, z=z, u=u)
    wo, so, _, _ = go(z=z, c=c, stop=torch.cat(stop_list, 1))
    _close(wave, wo, msg='wave')
    _close(s, so, msg='stop logits')


def test_train_loop_sampling_changes_no_training_bit(tmp_path):
    """eager TrainLoop with sample_every=1 (and audio every 2nd generator iteration) against the same loop without sampling:
    the same log and the same parameter bits; the callback saw every generator iteration"""
    import audiogan_amd as A
    from tests.test_loop import _setup
    B = 4
    words = (np.random.RandomState(0).randint(97, 123, size=(B, 5)), np.array([5, 3, 4, 2]))
    res, seen = [], []
    for sampling in (False, True):
        mk, mods, _ = _setup(A, torch.device('cpu'), False, tmp_path, B)
        torch.manual_seed(7)
        kw = dict(sample_every=1, sample_words=words, sample_seed=3, sample_dir=str(tmp_path / 'wav'), audio_every=2,
                  on_sample=lambda n, w, ln, sl: seen.append((n, tuple(w.shape), ln.clone(), len(sl)))) if sampling else {}
        lp = mk(fixed_critic_iter=2, gencatchup=1, checkpoint_every=0, **kw)
        for _ in range(3):
            lp.outer()
        res.append((list(lp.log), [p.detach().clone() for m in mods for p in m.parameters()]))
        if sampling:
            assert lp.last_sample_u is not None and tuple(lp.last_sample_u.shape) == (lp.nframes, B)
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)
    assert [n for n, *_ in seen] == [1, 2, 3]
    for n, shp, ln, nstop in seen:
        assert shp[0] == B and shp[1] == int(ln.max()) == nstop * 32 and int(ln.min()) >= 32
    wavs = sorted(os.listdir(tmp_path / 'wav'))
    assert wavs == ['sample-00002-%d.wav' % i for i in range(B)]


def _parse_wav(path):
    raw = open(path, 'rb').read()
    assert raw[:4] == b'RIFF' and raw[8:12] == b'WAVE' and struct.unpack('<I', raw[4:8])[0] == len(raw) - 8
    chunks, o = {}, 12
    while o < len(raw):
        cid, n = raw[o:o + 4], struct.unpack('<I', raw[o + 4:o + 8])[0]
        chunks[cid] = raw[o + 8:o + 8 + n]
        o += 8 + n + (n & 1)
    return chunks


def test_write_wav_round_trip(tmp_path):
    from audiogan_amd.audio import write_wav
    x = np.random.RandomState(1).uniform(-1, 1, 1001).astype(np.float32)
    p = str(tmp_path / 'a.wav')
    write_wav(p, torch.from_numpy(x), sr=8000)
    ch = _parse_wav(p)
    tag, nch, sr, byte_rate, align, bits = struct.unpack('<HHIIHH', ch[b'fmt '][:16])
    assert (tag, nch, sr, byte_rate, align, bits) == (3, 1, 8000, 32000, 4, 32)
    assert ch[b'data'] == x.astype('<f4').tobytes()
    assert np.array_equal(np.frombuffer(ch[b'data'], dtype='<f4'), x)
    write_wav(p, x[:0], sr=16000)
    ch = _parse_wav(p)
    assert struct.unpack('<I', ch[b'fmt '][4:8])[0] == 16000 and ch[b'data'] == b''

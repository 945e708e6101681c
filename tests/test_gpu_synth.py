"""Sentence synthesis on the GPU (-m gpu): ag_join_facts and ag_join_clips under the checkers of tests/join_model.py (bit for bit
against the model, NaN-filled guarded destinations, both store forms, a side stream), the library's refusals, ``Voice`` on a
real Generator and Embedder against ``synth.join_host`` on the rows it generated, trimming, rendering, and a checkpoint's
averaged weights through ``Voice.from_checkpoint``.  Every comparison of samples is bit equality."""
import math
import os

import numpy as np
import pytest
import torch

from audiogan_amd import audio, synth
from tests import join_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


def test_facts_on_the_rows(K):
    assert M.check_facts(K.join_facts, on=_cuda) == 8
    assert K.lib.ag_last_kernel().decode() == 'join_facts_kernel'


@pytest.mark.parametrize('values', M.VALUES)
def test_clips_on_the_table_in_both_store_forms(K, values):
    """every case at its own pitch, then 16-byte aligned, then at an odd pitch one float off: the same bits, both kernels"""
    seen = set()
    for case in M.clip_cases():
        for form in (None, 'vector', 'scalar'):
            M.run_clips(K.join_clips, case, values, on=_cuda, form=form)
            seen.add((form, K.lib.ag_last_kernel().decode()))
    assert {k for _, k in seen} == {'join_clips_kernel<1>', 'join_clips_kernel<0>'}
    assert ('vector', 'join_clips_kernel<0>') not in seen and ('scalar', 'join_clips_kernel<1>') not in seen


def test_clips_on_a_side_stream(K):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name in ('overlap_edge', 'shared_rows', 'scan300'):
            case = [c for c in M.clip_cases() if c.name == name][0]
            M.run_clips(K.join_clips, case, 'randn', on=_cuda)
        M.check_facts(K.join_facts, on=_cuda)
    side.synchronize()


def test_the_library_refuses(K):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).cuda()          # noqa: E731
    i32 = torch.int32
    wave, off, n, gain = z(3, 16), z(3, dt=i32), z(3, dt=i32), z(3)
    out = z(1, 64)
    with pytest.raises(ValueError, match='ag_join_max_segments'):          # 1025 segments in one sentence
        K.join_clips(wave, off, n, gain, z(1025, dt=i32), z(1025, dt=i32), torch.tensor([0, 1025], dtype=i32).cuda(),
                     K.join_ramp(4, 'cuda'), out)
    with pytest.raises(ValueError, match='a fade of 4097'):
        K.join_clips(wave, off, n, gain, z(2, dt=i32), z(2, dt=i32), torch.tensor([0, 2], dtype=i32).cuda(), z(4097), out)
    with pytest.raises(ValueError, match='pitch'):
        K.join_clips(wave, off, n, gain, z(2, dt=i32), z(2, dt=i32), torch.tensor([0, 1, 2], dtype=i32).cuda(), z(4),
                     torch.zeros(100).cuda().as_strided((2, 64), (32, 1)))
    with pytest.raises(RuntimeError):
        K.join_facts(wave.cpu(), off, n)
    with pytest.raises(TypeError):
        K.join_facts(wave, off.long(), n)
    # what the tables hold cannot send a load outside the rows: a row index out of range is an empty segment
    wave = torch.randn(3, 16).cuda()
    n = torch.tensor([16, 16, 16], dtype=i32).cuda()
    out = torch.full((1, 64), float('nan')).cuda()
    _, ln = K.join_clips(wave, off, n, torch.ones(3).cuda(), torch.tensor([0, 7, -1, 2], dtype=i32).cuda(), z(4, dt=i32),
                         torch.tensor([0, 4], dtype=i32).cuda(), z(0), out)
    assert int(ln[0]) == 32 and torch.equal(out[0, :32].cpu(), torch.cat([wave[0], wave[2]]).cpu()) and not out[0, 32:].any()


# ---- the voice on real modules ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models(K):
    import audiogan_amd as A
    torch.manual_seed(12)
    g = A.Generator(frame_size=64, state_size=128, noise_size=16, embed_size=16).cuda()
    e = A.Embedder(output_size=16, char_embed_size=8, num_layers=1, num_chars=256).cuda()
    return A, g, e


TEXT = ['the cat sat', 'on', 'a mat today']


def test_say_batch_is_join_host_on_the_rows_it_generated(K, models):
    _, g, e = models
    v = synth.Voice(g, e, 'cuda', max_samples=1024, fade_ms=2.0, pause_ms=10.0)
    out, ln, marks = v.say_batch(TEXT, seed=3)
    assert out.is_cuda and out.dtype == torch.float32 and out.size(0) == 3 and ln.dtype == np.int64
    out2, ln2, marks2 = v.say_batch(TEXT, seed=3)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and np.array_equal(ln, ln2) and marks == marks2
    flat = [w for s in TEXT for w in s.split()]
    rows, n = v._rows(flat, 3)
    R = len(flat)
    rows_h, n_h, off_h = rows.cpu().numpy(), n.cpu().numpy(), np.zeros(R, dtype=np.int32)
    gain, bad = synth.facts_host(rows_h, off_h, n_h, 0.9)
    assert not bad.any()
    want, want_len = synth.join_host(rows_h, off_h, n_h, gain, np.arange(R), np.full(R, v.join), [0, 3, 4, 7],
                                     K.join_ramp(v.fade).numpy(), out.size(1))
    assert np.array_equal(ln, want_len)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    for s in range(3):
        st, total = synth.join_plan([z - a for _, a, z in marks[s]], [v.join] * len(marks[s]))
        assert st == [a for _, a, _ in marks[s]] and total == ln[s]
    vo = synth.Voice(g, e, 'cuda', max_samples=1024, fade_ms=2.0, overlap_ms=4.0, peak=None)
    out, ln, marks = vo.say_batch(TEXT, seed=3)
    want, want_len = synth.join_host(rows_h, off_h, n_h, np.ones(R, np.float32), np.arange(R), np.full(R, vo.join), [0, 3, 4, 7],
                                     K.join_ramp(vo.fade).numpy(), out.size(1))
    assert np.array_equal(ln, want_len) and np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


def test_trim_against_activity64_on_the_same_rows(K, models):
    _, g, e = models
    opts = dict(max_samples=2048, fade_ms=0.0, pause_ms=1.0, peak=None, activity=dict(top_db=6.0, min_run_ms=10.0, pad_ms=0.0))
    v = synth.Voice(g, e, 'cuda', trim=True, **opts)
    out, ln, marks = v.say_batch(['ab cd ef'], seed=8)
    rows, n = v._rows(['ab', 'cd', 'ef'], 8)
    rows_h, n_h = rows.cpu().numpy(), n.cpu().numpy()
    segs = audio.activity64(rows_h, n_h, **opts['activity'])
    for r, ((_, a, z), seg) in enumerate(zip(marks[0], segs)):
        lo, hi = (int(seg[0, 0]), int(seg[-1, 1])) if len(seg) else (0, int(n_h[r]))
        assert z - a == hi - lo
        assert np.array_equal(out[0, a:z].cpu().numpy().view(np.int32), rows_h[r, lo:hi].view(np.int32))


def test_render_to_16k_pcm16(K, models, tmp_path):
    _, g, e = models
    v = synth.Voice(g, e, 'cuda', max_samples=512)
    wave, marks = v.say('hello you', seed=1)
    p = os.path.join(tmp_path, 'a.wav')
    assert synth.render(p, wave, sr_out=16000, fmt='pcm16') == math.ceil(wave.numel() * 2)
    assert K.lib.ag_last_kernel().decode() == 'resample_poly_kernel'
    data, sr = audio.read_wav(p)
    assert sr == 16000 and data.dtype == np.int16 and data.shape == (math.ceil(wave.numel() * 2), 1) and data.any()


def test_from_checkpoint_says_what_the_averaged_modules_say(K, models, tmp_path):
    A, g, e = models
    from audiogan_amd import checkpoint, optim
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e.parameters()), 'rmsprop', 1e-4)
    ema = optim.EMA(opt_g, decay=0.5, warmup=False)
    with torch.no_grad():
        for p in list(g.parameters()) + list(e.parameters()):
            p.mul_(1.25)
    ema.update()
    prefix = os.path.join(tmp_path, 'ck')
    checkpoint.save(prefix, 11, g=g, e_g=e, ema=ema)
    v = synth.Voice.from_checkpoint(prefix, 11, device='cuda', max_samples=512, fade_ms=1.0, pause_ms=5.0)
    assert v.info['weights'] == 'ema' and v.info['kind'] == 'lstm' and v.info['generator']['struct'] == [(17, 8, 128, 16), (9, 4, 64, 32), (9, 4, 64, 32), (9, 4, 32, 32)]
    out, ln, marks = v.say_batch(TEXT, seed=2)
    with ema.applied():
        want, want_len, want_marks = synth.Voice(g, e, 'cuda', max_samples=512, fade_ms=1.0, pause_ms=5.0).say_batch(TEXT, seed=2)
    assert np.array_equal(ln, want_len) and marks == want_marks and torch.equal(out.view(torch.int32), want.view(torch.int32))
    raw, _, _ = synth.Voice(g, e, 'cuda', max_samples=512, fade_ms=1.0, pause_ms=5.0).say_batch(TEXT, seed=2)
    assert not torch.equal(raw, want)

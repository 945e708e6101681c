"""Sentence synthesis on the host: the plan, the ramp, ``synth.join_host`` / ``facts_host`` against the model of
tests/join_model.py over the whole case table (bit for bit), the checkers against mutants of the model, the wrappers' and the
library's refusals, ``models_from_checkpoint``, ``Voice`` with a stub generator and a stub embedder, PCM16 output, the CLI and the
round trip through ``ingest``.  The launches themselves: tests/test_gpu_synth.py."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import audiogan_amd.kernels as K
from audiogan_amd import _lib, audio, ingest, synth
from tests import join_model as M
from tests import kernel_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan and the ramp -----------------------------------------------------------------------------------------------
def test_join_plan_by_hand():
    assert synth.join_plan([], []) == ([], 0)
    assert synth.join_plan([5], [99]) == ([0], 5)                                   # the last join is ignored
    assert synth.join_plan([5, 7], [3, 0]) == ([0, 8], 15)                          # a pause
    assert synth.join_plan([1040, 100], [-40, 0]) == ([0, 1000], 1100)              # an overlap
    assert synth.join_plan([13, 40], [-50, 0]) == ([0, 7], 47)                      # ov = min(50, 6, 20) = 6
    assert synth.join_plan([40, 1], [-50, 0]) == ([0, 40], 41)                      # ov = min(50, 20, 0) = 0
    assert synth.join_plan([40, 0, 40], [-50, -50, 0]) == ([0, 40, 40], 80)         # nothing overlaps across an empty segment
    assert synth.join_plan([0, 7, 0], [3, -2, 5]) == ([0, 3, 10], 10)
    assert synth.join_plan(np.array([4, 4], dtype=np.int32), np.array([-2, 0], dtype=np.int32)) == ([0, 2], 6)


@pytest.mark.parametrize('F', [1, 2, 7, 40, 4096])
def test_ramp_rises_and_is_complementary(F):
    r = K.join_ramp(F)
    assert r.dtype == torch.float32 and tuple(r.shape) == (F,) and K.join_ramp(F) is r          # cached
    assert torch.equal(r, M.ramp(F))
    assert bool((r[1:] > r[:-1]).all()) and 0 < float(r[0]) and float(r[-1]) < 1
    assert float((r.double() + r.flip(0).double() - 1).abs().max()) <= 1e-7
    assert K.join_ramp(0).numel() == 0
    with pytest.raises(ValueError):
        K.join_ramp(4097)


# ---- the host path against the model ---------------------------------------------------------------------------------------
def host_facts(wave, off, n, target=0.0):
    g, b = synth.facts_host(wave.numpy(), off.numpy(), n.numpy(), target)
    return torch.from_numpy(g), torch.from_numpy(b)


def host_clips(wave, off, n, gain, seg_row, join, sent_ptr, ramp, out, out_len=None, pause_max=0):
    o, ln = synth.join_host(wave.numpy(), off.numpy(), n.numpy(), gain.numpy(), seg_row.numpy(), join.numpy(), sent_ptr.numpy(),
                            ramp.numpy(), out.size(1))
    out.copy_(torch.from_numpy(o))
    out_len.copy_(torch.from_numpy(ln))
    return out, out_len


def test_facts_host_against_the_model():
    assert M.check_facts(host_facts) == 8


@pytest.mark.parametrize('values', M.VALUES)
def test_join_host_against_the_model_over_the_table(values):
    for case in M.clip_cases():
        M.run_clips(host_clips, case, values)
    # the two store forms of the launch are one rule: any pitch and offset of the destination
    M.run_clips(host_clips, M.clip_cases()[2], values, form='scalar')


def test_the_table_covers_what_it_says():
    cases = {c.name: c for c in M.clip_cases()}
    assert len(cases) == len(M.clip_cases()) == 16
    assert max(len(s) for s in cases['scan1024'].sents) == M.MAX_SEG == K.JOIN_MAX_SEGMENTS
    assert cases['long_ramp'].F == K.JOIN_MAX_FADE
    assert cases['odd_pitch'].pitch % 2 == 1 and cases['odd_pitch'].shift == 1
    _, ln = M._expected(cases['truncated'], 'int')
    assert int(ln[0]) == 160 > cases['truncated'].O_cap
    _, ln = M._expected(cases['ov_clamps'], 'int')
    assert ln.tolist() == [47, 41, 80]
    out, ln = M._expected(cases['pause_edge'], 'randn')
    assert int(ln[0]) == 1060 and not out[0, 1020:1030].any() and bool(out[0, 1019] != 0) and bool(out[0, 1030] != 0)


@pytest.mark.parametrize('mutant', M.CLIP_MUTANTS)
def test_checkers_reject_mutants_of_the_model(mutant):
    def fn(*a, **k):
        return M.join_clips(*a, mutate=mutant, **k)
    caught = []
    for values in M.VALUES:
        for case in M.clip_cases():
            try:
                M.run_clips(fn, case, values)
            except AssertionError as e:
                caught.append((case.name, values, e.args[0][0] if e.args and isinstance(e.args[0], tuple) else str(e)))
    assert caught, mutant
    names = {c[0] for c in caught}
    want = dict(overlap_without_half='ov_clamps', fade_index_unscaled='fade_clip', fma='overlap_edge',
                out_len_truncated='truncated', pause_not_zeroed='pause_edge')[mutant]
    assert want in names, (mutant, sorted(names))


# ---- refusals --------------------------------------------------------------------------------------------------------------
class OnDevice(object):
    """a host tensor that says it lives on the device: what the wrappers' checks read before any launch"""

    def __init__(self, t):
        self.t, self.is_cuda = t, True

    def __getattr__(self, name):
        return getattr(self.t, name)


def _wrapper_args(**swap):
    z = dict(wave=torch.zeros(3, 16), off=torch.zeros(3, dtype=torch.int32), n=torch.zeros(3, dtype=torch.int32),
             gain=torch.ones(3), seg_row=torch.zeros(4, dtype=torch.int32), join=torch.zeros(4, dtype=torch.int32),
             sent_ptr=torch.tensor([0, 2, 4], dtype=torch.int32), ramp=torch.zeros(4), out=torch.zeros(2, 40),
             out_len=torch.zeros(2, dtype=torch.int64))
    z.update(swap)
    return [OnDevice(z[k]) for k in ('wave', 'off', 'n', 'gain', 'seg_row', 'join', 'sent_ptr', 'ramp', 'out', 'out_len')]


@pytest.mark.parametrize('name,bad,exc', [
    ('wave', torch.zeros(3, 16, dtype=torch.float64), TypeError),
    ('off', torch.zeros(3, dtype=torch.int64), TypeError),
    ('n', torch.zeros(3), TypeError),
    ('gain', torch.ones(3, dtype=torch.float16), TypeError),
    ('seg_row', torch.zeros(4, dtype=torch.int64), TypeError),
    ('sent_ptr', torch.tensor([0, 2, 4]), TypeError),
    ('out_len', torch.zeros(2, dtype=torch.int32), TypeError),
    ('out', torch.zeros(2, 40, dtype=torch.bfloat16), TypeError),
    ('wave', torch.zeros(16, 3).t(), ValueError),                                   # not unit stride along the samples
    ('off', torch.zeros(4, dtype=torch.int32), ValueError),                         # not one per row
    ('gain', torch.ones(2), ValueError),
    ('join', torch.zeros(5, dtype=torch.int32), ValueError),
    ('out', torch.zeros(3, 40), ValueError),                                        # not one row per sentence
    ('out', torch.zeros(2, 80)[:, ::2], ValueError),
    ('out_len', torch.zeros(3, dtype=torch.int64), ValueError),
    ('ramp', torch.zeros(2, 2), ValueError),
])
def test_wrappers_refuse_before_the_launch(name, bad, exc):
    with pytest.raises(exc) as e:
        K.join_clips(*_wrapper_args(**{name: bad}))
    assert name in str(e.value) or name.split('_')[0] in str(e.value), str(e.value)
    if name in ('wave', 'off', 'n'):
        with pytest.raises(exc):
            K.join_facts(*_wrapper_args(**{name: bad})[:3])


def test_wrappers_refuse_host_tensors():
    a = _wrapper_args()
    with pytest.raises(RuntimeError, match='wave must be a CUDA'):
        K.join_facts(torch.zeros(3, 16), a[1], a[2])
    with pytest.raises(RuntimeError, match='out must be a CUDA'):
        K.join_clips(*a[:8], torch.zeros(2, 40))
    assert K.JOIN_MAX_SEGMENTS == 1024 and not hasattr(K.join_clips, 'timed_name')


def test_launchers_refuse_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    buf = (C.c_char * 256)()
    p = C.addressof(buf) // 16 * 16 + 16

    def clips(**kw):
        a = dict(wave=p, ld=16, L_in=16, off=p, n=p, gain=p, R=3, seg_row=p, join=p, sent_ptr=p, K=4, S=2, pause_max=0, ramp=p,
                 F=4, out=p, ld_out=40, O_cap=40, out_len=p)
        a.update(kw)
        return K.lib.ag_join_clips(a['wave'], a['ld'], a['L_in'], a['off'], a['n'], a['gain'], a['R'], a['seg_row'], a['join'],
                                   a['sent_ptr'], a['K'], a['S'], a['pause_max'], a['ramp'], a['F'], a['out'], a['ld_out'],
                                   a['O_cap'], a['out_len'], None)
    for bad in (dict(K=1025, S=1), dict(K=2049, S=2), dict(F=4097), dict(F=-1), dict(S=-1), dict(S=65536, K=0), dict(R=-1),
                dict(L_in=-1), dict(O_cap=-1), dict(pause_max=-1), dict(ld=15), dict(ld_out=39), dict(out=None),
                dict(sent_ptr=None), dict(out_len=None), dict(seg_row=None), dict(gain=None), dict(ramp=None),
                dict(K=1024, S=1, L_in=1 << 21, ld=1 << 21), dict(K=2, L_in=1 << 30, ld=1 << 30, pause_max=1 << 30)):
        assert clips(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_join_clips'), bad
    assert clips(K=1025, S=1) == _lib.AG_ERR_ARG and b'ag_join_max_segments' in K.lib.ag_last_error()
    assert clips(S=0, K=0) == _lib.AG_OK and clips(S=0, K=0, out=None, sent_ptr=None) == _lib.AG_OK

    def facts(**kw):
        a = dict(wave=p, ld=16, L_in=16, off=p, n=p, R=3, target=0.9, gain=p, bad=p)
        a.update(kw)
        return K.lib.ag_join_facts(a['wave'], a['ld'], a['L_in'], a['off'], a['n'], a['R'], a['target'], a['gain'], a['bad'], None)
    for bad in (dict(R=-1), dict(L_in=-1), dict(ld=15), dict(wave=None), dict(off=None), dict(n=None), dict(gain=None),
                dict(bad=None), dict(target=float('nan'))):
        assert facts(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_join_facts'), bad
    assert facts(R=0) == _lib.AG_OK and facts(R=0, wave=None, gain=None) == _lib.AG_OK
    header = open(os.path.join(ROOT, 'include', 'audiogan_hip.h')).read()
    for sym in ('ag_join_max_segments', 'ag_join_facts', 'ag_join_clips'):
        assert sym in _lib.SIGNATURES and 'int %s(' % sym in header
    assert 'join.hip' in open(os.path.join(ROOT, 'audiogan_amd', 'csrc', 'Makefile')).read()


# ---- the modules back from a checkpoint ------------------------------------------------------------------------------------
def _small(A, kind):
    torch.manual_seed(4)
    if kind == 'gru':
        g, gargs = A.GRUGenerator(16, 6, 5, 24, struct=[[9, 4, 8, 4]]), dict(
            frame_size=16, embed_size=6, noise_size=5, state_size=24, struct=[(9, 4, 8, 4)])
    else:
        g, gargs = A.Generator(16, 6, 5, 24, 2, struct=[[9, 4, 8, 4], [5, 2, 6, 3]]), dict(
            frame_size=16, embed_size=6, noise_size=5, state_size=24, num_layers=2, struct=[(9, 4, 8, 4), (5, 2, 6, 3)])
    return g, A.Embedder(6, 4, 2, 40), gargs, dict(output_size=6, char_embed_size=4, num_layers=2, num_chars=40)


@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_models_from_checkpoint_infers_the_arguments(tmp_path, monkeypatch, kind):
    kernel_model.install(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd import checkpoint
    g, e, gargs, eargs = _small(A, kind)
    prefix = os.path.join(tmp_path, 'm')
    checkpoint.save(prefix, 7, g=g, e_g=e)
    with pytest.warns(UserWarning, match='no averaged weights'):          # the EMA fallback warns, once
        g2, e2, info = synth.models_from_checkpoint(prefix, 7, device='cpu')
    assert info == dict(weights='plain', kind=kind, generator=gargs, embedder=eargs)
    assert type(g2) is type(g) and isinstance(e2, A.Embedder)
    for m, m2 in ((g, g2), (e, e2)):
        sd, sd2 = m.state_dict(), m2.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert synth.models_from_checkpoint(prefix, 7, use_ema=False, device='cpu')[2]['weights'] == 'plain'
        # averaged files, when they are there, are the ones read
        for role, m in (('genema', g), ('egema', e)):
            torch.save({k: v * 0.5 if v.is_floating_point() else v for k, v in m.state_dict().items()},
                       '%s-%s-%05d' % (prefix, role, 7))
        g3, _, info3 = synth.models_from_checkpoint(prefix, 7, device='cpu')
    assert info3['weights'] == 'ema' and not [w for w in seen if 'averaged' in str(w.message)]
    assert torch.equal(g3.state_dict()['proj.module.weight_v'], g.state_dict()['proj.module.weight_v'] * 0.5)
    v = synth.Voice.from_checkpoint(prefix, 7, use_ema=False, device='cpu', max_samples=64)
    assert v.info['kind'] == kind and v.num_chars == 40 and v.frame == 16 and v.frames == 4


def test_models_from_checkpoint_names_what_it_refuses(tmp_path, monkeypatch):
    kernel_model.install(monkeypatch)
    import audiogan_amd as A
    g, e, _, _ = _small(A, 'lstm')
    prefix = os.path.join(tmp_path, 'm')

    def write(gen_edit=None, eg_edit=None):
        gs, es = dict(g.state_dict()), dict(e.state_dict())
        (gen_edit or (lambda sd: None))(gs)
        (eg_edit or (lambda sd: None))(es)
        torch.save(gs, prefix + '-gen-00003')
        torch.save(es, prefix + '-eg-00003')

    def conv_k(sd):
        sd['dense_res_gen.1.module.conv.weight_v'] = torch.zeros(6, 5, 7)
    write(conv_k)
    with pytest.raises(ValueError, match=r"dense_res_gen\.1\.module\.conv\.weight_v' has shape \(6, 5, 7\)"):
        synth.models_from_checkpoint(prefix, 3, use_ema=False, device='cpu')

    def narrow(sd):
        sd['rnn.0.module.weight_ih_v'] = torch.zeros(96, 20)
    write(narrow)
    with pytest.raises(ValueError, match=r"rnn\.0\.module\.weight_ih_v has shape \(96, 20\).*noise size of -2"):
        synth.models_from_checkpoint(prefix, 3, use_ema=False, device='cpu')

    def rows(sd):
        sd['rnn.0.module.weight_ih_v'] = torch.zeros(50, 27)
    write(rows)
    with pytest.raises(ValueError, match=r"rnn\.0\.module\.weight_ih_v has shape \(50, 27\)"):
        synth.models_from_checkpoint(prefix, 3, use_ema=False, device='cpu')

    def no_embed(sd):
        del sd['embed.module.weight']
    write(None, no_embed)
    with pytest.raises(ValueError, match=r"no tensor 'embed\.module\.weight'"):
        synth.models_from_checkpoint(prefix, 3, use_ema=False, device='cpu')
    # a wrong guess cannot load silently: the strict load has the last word
    def extra(sd):
        sd['stray'] = torch.zeros(1)
    write(extra)
    with pytest.raises(RuntimeError, match='stray'):
        synth.models_from_checkpoint(prefix, 3, use_ema=False, device='cpu')


# ---- the voice, on stubs ---------------------------------------------------------------------------------------------------
class StubG(object):
    """clips that depend on nothing but their own row of c, z and u: frames of 8 samples, 1 .. T of them by the first uniform"""
    _frame_size, _noise_size = 8, 3

    def __init__(self, nan_len=None):
        self.calls, self.nan_len = [], nan_len

    def generate(self, c, length=None, z=None, u=None):
        B, T, _ = z.shape
        assert tuple(u.shape) == (T, B) and length == T * 8
        self.calls.append(B)
        first = (1 + (u[0] * T).long()).clamp(max=T)
        i = torch.arange(T * 8, dtype=torch.float32)
        wave = torch.sin(i[None, :] * (0.05 + 0.01 * c[:, 1:2]) + z[:, :, 0].repeat_interleave(8, 1)) * (0.2 + 0.01 * c[:, 0:1])
        wave = wave + 0.001 * z[:, :, 1].repeat_interleave(8, 1) + 1e-3
        if self.nan_len is not None:
            wave[c[:, 1] == self.nan_len, 3] = float('nan')
        t_eff = int(first.max())
        return wave[:, :t_eff * 8], None, None, first * 8


def stub_e(cseq, clen):
    return torch.stack([cseq.float().sum(1) % 17, clen.float()], 1)


def _voice(**kw):
    kw = dict(dict(max_samples=64, fade_ms=0.5, pause_ms=2.0), **kw)
    return synth.Voice(StubG(kw.pop('nan_len', None)), stub_e, 'cpu', **kw)


def test_voice_same_seed_same_bits_and_marks_match_the_plan():
    v = _voice()
    assert (v.fade, v.join, v.frames, v.chunk) == (4, 16, 8, 64)
    state = torch.get_rng_state()
    text = ['the quick brown fox', '', ['jumps', 'over'], 'dog']
    out, ln, marks = v.say_batch(text, seed=5)
    assert torch.equal(torch.get_rng_state(), state)          # no global RNG moved
    out2, ln2, marks2 = v.say_batch(text, seed=5)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and np.array_equal(ln, ln2) and marks == marks2
    out3, _, _ = v.say_batch(text, seed=6)
    assert not torch.equal(out, out3)
    assert out.dtype == torch.float32 and out.size(0) == 4 and ln.dtype == np.int64 and ln[1] == 0 and marks[1] == []
    assert [w for w, _, _ in marks[0]] == ['the', 'quick', 'brown', 'fox'] and [w for w, _, _ in marks[2]] == ['jumps', 'over']
    for s in range(4):
        n = [z - a for _, a, z in marks[s]]
        st, total = synth.join_plan(n, [16] * len(n))
        assert [a for _, a, _ in marks[s]] == st and total == ln[s]
        assert all(k % 8 == 0 and 8 <= k <= 64 for k in n)
        assert not out[s, int(ln[s]):].any()
        for _, a, z in marks[s]:
            assert 0.3 < float(out[s, a:z].abs().max()) <= 0.9 * (1 + 1e-6)          # every word scaled to the peak
        for (_, _, z), (_, a, _) in zip(marks[s], marks[s][1:]):
            assert a - z == 16 and not out[s, z:a].any()
    wave, m = v.say('jumps over', seed=5)
    assert len(m) == 2 and wave.numel() == m[-1][2]
    # overlaps: the plan's clamp shows in the marks
    vo = _voice(overlap_ms=3.0)
    assert vo.join == -24
    _, lno, mo = vo.say_batch(['a b c d e'], seed=2)
    n = [z - a for _, a, z in mo[0]]
    assert synth.join_plan(n, [-24] * 5) == ([a for _, a, _ in mo[0]], lno[0]) and lno[0] < sum(n)


def test_voice_chunks_of_64_do_not_change_the_bits():
    words = ['w%d' % i for i in range(70)]
    v = _voice()
    out, ln, marks = v.say_batch([words], seed=3)
    assert v.g.calls == [64, 6]
    whole = _voice()
    whole.chunk = 128
    out2, ln2, marks2 = whole.say_batch([' '.join(words)], seed=3)
    assert whole.g.calls == [70]
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and np.array_equal(ln, ln2) and marks == marks2


def test_voice_refusals():
    with pytest.raises(ValueError, match="'abc'"):
        _voice(nan_len=3).say_batch(['it is abc today'])
    with pytest.raises(ValueError, match='caf'):
        _voice().say('a cafē b')          # a character outside Latin-1
    with pytest.raises(ValueError, match='1025 words'):
        _voice().say_batch([['a'] * 1025])
    with pytest.raises(ValueError, match='fade'):
        _voice(fade_ms=600.0)
    out, ln, marks = _voice().say_batch([])
    assert tuple(out.shape)[0] == 0 and len(ln) == 0 and marks == []


def test_voice_trim_cuts_to_the_active_stretch():
    class Padded(StubG):
        def generate(self, c, length=None, z=None, u=None):
            wave, a, b, ln = super().generate(c, length, z, torch.full_like(u, 0.99))
            wave = wave.clone()
            wave[:, :400] = 0
            wave[:, 1200:] = 0
            return wave, a, b, ln
    opts = dict(max_samples=1600, fade_ms=0.0, pause_ms=1.0, peak=None)
    v = synth.Voice(Padded(), stub_e, 'cpu', trim=True, **opts)
    out, ln, marks = v.say_batch(['ab cd'], seed=1)
    plain = synth.Voice(Padded(), stub_e, 'cpu', **opts)
    rows, n = plain._rows(['ab', 'cd'], 1)
    segs = audio.activity64(rows.numpy(), n.numpy())
    for (_, a, z), seg, r in zip(marks[0], segs, range(2)):
        assert len(seg) == 1 and z - a == seg[0, 1] - seg[0, 0] < 1600
        assert torch.equal(out[0, a:z], rows[r, seg[0, 0]:seg[0, 1]])


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_write_wav_pcm16_and_the_default_bytes(tmp_path):
    p = os.path.join(tmp_path, 'a.wav')
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 1e-5, 0.25], dtype=np.float32)
    audio.write_wav(p, x, sr=16000, fmt='pcm16')
    data, sr = audio.read_wav(p)
    assert sr == 16000 and data.dtype == np.int16 and data.shape == (9, 1)
    assert data[:, 0].tolist() == [0, 16384, -16384, 32767, -32767, 32767, -32768, 0, 8192]
    raw = open(p, 'rb').read()
    assert raw[20:22] == b'\x01\x00' and len(raw) == 44 + 18
    audio.write_wav(p, torch.tensor([1.0, -0.5]), sr=8000)
    want = (b'RIFF' + (50 + 8).to_bytes(4, 'little') + b'WAVEfmt ' + (18).to_bytes(4, 'little') + b'\x03\x00\x01\x00' +
            (8000).to_bytes(4, 'little') + (32000).to_bytes(4, 'little') + b'\x04\x00\x20\x00\x00\x00' + b'fact' +
            (4).to_bytes(4, 'little') + (2).to_bytes(4, 'little') + b'data' + (8).to_bytes(4, 'little') +
            b'\x00\x00\x80\x3f\x00\x00\x00\xbf')
    assert open(p, 'rb').read() == want
    audio.write_wav(p, torch.tensor([1.0, -0.5]), 8000, 'float32')
    assert open(p, 'rb').read() == want
    with pytest.raises(ValueError, match='pcm24'):
        audio.write_wav(p, x, fmt='pcm24')


def test_cli_writes_files_numbers_sentences_and_marks(tmp_path):
    v = _voice()
    out = os.path.join(tmp_path, 'say.wav')
    assert synth.main(['--text', 'hello there', '--out', out, '--seed', '4'], voice=v) == 0
    data, sr = audio.read_wav(out)
    wave, marks = v.say('hello there', seed=4)
    assert sr == 16000 and data.dtype == np.int16 and data.shape == (2 * wave.numel(), 1)
    txt = os.path.join(tmp_path, 'lines.txt')
    with open(txt, 'w') as f:
        f.write('one two\n\nthree\n')
    calls = len(v.g.calls)
    tsv = os.path.join(tmp_path, 'marks.tsv')
    assert synth.main(['--text-file', txt, '--out', out, '--rate', '8000', '--format', 'float32', '--marks-out', tsv], voice=v) == 0
    assert len(v.g.calls) == calls + 1          # ONE say_batch, one chunk
    batch, ln, marks = v.say_batch(['one two', '', 'three'])
    for i in range(3):
        data, sr = audio.read_wav(os.path.join(tmp_path, 'say-%03d.wav' % i))
        assert sr == 8000 and data.dtype == np.float32 and np.array_equal(data[:, 0], batch[i, :ln[i]].numpy())
    lines = [line.rstrip('\n').split('\t') for line in open(tsv) if not line.startswith('#')]
    assert [(os.path.basename(p), w) for p, w, _, _ in lines] == [('say-000.wav', 'one'), ('say-000.wav', 'two'), ('say-002.wav', 'three')]
    assert lines[1][2:] == ['%.6f' % ((marks[0][1][1] + 0.5) / 8000), '%.6f' % ((marks[0][1][2] + 0.5) / 8000)]
    with pytest.raises(SystemExit):
        synth.main(['--out', out], voice=v)


def test_round_trip_through_ingest(tmp_path):
    """rendered at the models' rate with no fades, no normalisation and a pause, the marks cut every word back out bit for bit"""
    v = _voice(fade_ms=0.0, peak=None, pause_ms=3.0)
    txt, out, tsv = (os.path.join(tmp_path, n) for n in ('t.txt', 'r.wav', 'm.tsv'))
    with open(txt, 'w') as f:
        f.write('alpha beta gamma\nbeta delta\n')
    assert synth.main(['--text-file', txt, '--out', out, '--rate', '8000', '--format', 'float32', '--marks-out', tsv,
                       '--seed', '9'], voice=v) == 0
    store, report = ingest.build_store(ingest.read_manifest(tsv), device='cpu')
    flat = ['alpha', 'beta', 'gamma', 'beta', 'delta']
    rows, n = v._rows(flat, 9)
    assert report['kept'] == dict(alpha=1, beta=2, gamma=1, delta=1) and not any(report['dropped'].values())
    seen = {}
    for r, w in enumerate(flat):
        i = seen.get(w, 0)
        seen[w] = i + 1
        want = rows[r, :int(n[r])].numpy()
        assert np.array_equal(store[w][i, :len(want)].view(np.int32), want.view(np.int32)) and not store[w][i, len(want):].any()

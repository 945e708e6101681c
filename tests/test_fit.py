"""``python -m audiogan_amd.fit`` on the host: the reference's flags and defaults, the combinations the parser refuses,
``fit.build`` on a synthetic store of two-tone words, ``--loaditerations`` on a checkpoint ``checkpoint.save`` wrote, and ``main``
for one pass on the kernel models at the small widths of tests/test_loop.py (which runs ``TrainLoop`` on the CPU the same way).
The command on the HIP kernels: tests/test_gpu_fit.py."""
import json
import os

import numpy as np
import pytest
import torch

from audiogan_amd import fit, ingest, sheet
from tests import ema_model, kernel_model, summary_model
from tests.test_sheet import read_png

# audiogan.py:554-579, as the issue lists them
REFERENCE_DEFAULTS = dict(
    critic_iter=100, rnng_layers=1, rnnd_layers=1, framesize=200, noisesize=100, gstatesize=1024, dstatesize=1024, batchsize=32,
    dgradclip=1.0, ggradclip=0.1, dlr=1e-4, glr=1e-4, modelnamesave='', modelnameload='', loaditerations=0, gencatchup=1,
    dataset='dataset.h5', embedsize=100, minwordlen=1, maxlen=40000, noisescale=0.01, g_optim='boundary_seeking', require_acc=0.5)
WORDS = ['alpha', 'beta', 'gamma', 'delta', 'epsil', 'zetaa', 'etaaa', 'theta', 'iotaa', 'kappa', 'lambd']
# the small widths of tests/test_loop.py
SMALL = ['--framesize', '32', '--noisesize', '8', '--gstatesize', '64', '--dstatesize', '64', '--embedsize', '8',
         '--charembedsize', '6', '--batchsize', '4', '--maxlen', '128', '--gstruct', '17,8,16,8;9,4,16,8', '--dstruct', '7,2,8;7,2,16']


def two_tone_store(words=WORDS, clips=4, maxlen=128, seed=0):
    """word -> float32 [clips, maxlen], zero padded: a tone that switches to a second one half way, both set by the word"""
    rs = np.random.RandomState(seed)
    store = {}
    for i, w in enumerate(words):
        arr = np.zeros((clips, maxlen), dtype=np.float32)
        for c in range(clips):
            n = int(rs.randint(maxlen // 3, maxlen + 1))
            t = np.arange(n)
            f = np.where(t < n // 2, 300.0 + 90.0 * i, 1500.0 + 110.0 * i)
            arr[c, :n] = 0.5 * np.sin(2 * np.pi * f * t / 8000.0) + 1e-3 * rs.standard_normal(n)
            arr[c, n - 1] = 0.25
        store[w] = arr
    return store


@pytest.fixture()
def store_path(tmp_path):
    p = os.path.join(tmp_path, 'words.npz')
    ingest.save_store(two_tone_store(), p)
    return p


def _models(monkeypatch):
    kernel_model.install(monkeypatch)
    ema_model.install(monkeypatch)
    summary_model.install(monkeypatch)


# ---- the parser -------------------------------------------------------------------------------------------------------------
def test_every_reference_flag_parses_to_the_references_default():
    a = fit.parse(['--outer', '3', '--device', 'cpu'])
    assert {n for n, _, _ in fit.REFERENCE_FLAGS} == set(REFERENCE_DEFAULTS) and len(fit.REFERENCE_FLAGS) == 23
    for name, want in REFERENCE_DEFAULTS.items():
        got = getattr(a, name)
        assert got == want and type(got) is type(want) or (name == 'dgradclip' and got == 1), (name, got, want)
    assert a.outer == 3 and a.stop == 'draw' and a.optim == 'rmsprop' and a.dtype == 'f32' and a.ema is None
    assert not (a.graphed or a.device_store or a.aligned or a.crossed) and a.fixed_critic_iter is None
    assert (a.checkpoint_every, a.sample_every, a.audio_every, a.sheet_every, a.eval_every, a.eval_batches, a.seed) == (500, 0, 0, 0, 0, 4, 0)
    # each takes a value of its type
    b = fit.parse(['--outer', '1', '--device', 'cpu', '--critic_iter', '7', '--dlr', '3e-4', '--g_optim', 'plain', '--maxlen', '0',
                   '--modelnamesave', 'run/m', '--gstruct', '17,8,16,8;9,4,16,8', '--sheet-every', '20'])
    assert (b.critic_iter, b.dlr, b.g_optim, b.maxlen, b.modelnamesave) == (7, 3e-4, 'plain', 0, 'run/m')
    assert b.gstruct == [[17, 8, 16, 8], [9, 4, 16, 8]] and b.sample_every == 20          # sheets are drawn from samples


@pytest.mark.parametrize('argv,says', [
    ([], '--outer'),                                                                # required: the reference loops forever
    (['--outer', '-1'], 'passes'),
    (['--outer', '1', '--graphed'], "graphed=True needs stop='never' and a CUDA device"),          # the loop's own reason
    (['--outer', '1', '--graphed', '--stop', 'never', '--device', 'cpu'], "graphed=True needs stop='never' and a CUDA device"),
    (['--outer', '1', '--device-store', '--device', 'cpu'], 'device-store'),
    (['--outer', '1', '--ema', '1.5'], 'decay must lie in [0, 1]'),
    (['--outer', '1', '--stop', 'sometimes'], 'invalid choice'),
    (['--outer', '1', '--optim', 'sgd'], 'invalid choice'),
    (['--outer', '1', '--aligned'], '--eval-every'),
    (['--outer', '1', '--crossed'], '--eval-every'),
    (['--outer', '1', '--eval-every', '5', '--eval-batches', '0'], 'at least one'),
    (['--outer', '1', '--sample-every', '3', '--sheet-every', '4', '--sample-dir', 's'], 'a multiple'),
    (['--outer', '1', '--sample-every', '3'], 'samples need a place'),
    (['--outer', '1', '--loaditerations', '5'], '--modelnameload'),
    (['--outer', '1', '--checkpoint-every', '-2'], 'negative'),
    (['--outer', '1', '--gstruct', '17,8;x'], 'structure'),
])
def test_the_parser_refuses(argv, says, capsys):
    with pytest.raises(SystemExit) as e:
        fit.parse(argv + ([] if '--device' in argv else ['--device', 'cpu']))
    assert e.value.code == 2 and says in capsys.readouterr().err


# ---- build ------------------------------------------------------------------------------------------------------------------
def test_build_yields_the_requested_shapes_and_the_references_optimiser_split(monkeypatch, store_path, tmp_path):
    _models(monkeypatch)
    import audiogan_amd as A
    from audiogan_amd import loop, optim
    a = fit.parse(SMALL + ['--outer', '1', '--device', 'cpu', '--dataset', store_path, '--rnng_layers', '2', '--optim', 'adam',
                           '--ema', '0.9', '--critic_iter', '5', '--require_acc', '0.7', '--gencatchup', '2',
                           '--modelnamesave', os.path.join(tmp_path, 'm'), '--sheet-every', '4', '--audio-every', '8', '--seed', '2'])
    s = fit.build(a)
    assert isinstance(s.g, A.Generator) and isinstance(s.d, A.Discriminator)
    assert (s.g._frame_size, s.g._noise_size) == (32, 8) and len(s.g.rnn) == 2 and s.d._state_size == 64
    assert tuple(s.g.rnn[0].module.weight_hh_v.shape) == (4 * 64, 64) and s.e_g._output_size == 8 and s.e_d._char_embed_size == 6
    same = lambda ps, qs: len(ps) == len(qs) and all(p is q for p, q in zip(ps, qs))      # noqa: E731
    assert same(s.opt_g.params, list(s.g.parameters()) + list(s.e_g.parameters()))          # audiogan.py:690-694
    assert same(s.opt_d.params, list(s.d.parameters()) + list(s.e_d.parameters()))
    assert isinstance(s.opt_g, optim.Adam) and (s.opt_g.lr, s.opt_d.lr) == (1e-4, 1e-4) and s.ema.opt is s.opt_g
    lp = s.loop
    assert isinstance(lp, loop.TrainLoop) and (lp.B, lp.maxlen, lp.L, lp.nframes) == (4, 128, 128, 4)
    assert (lp.critic_iter, lp.require_acc, lp.gencatchup, lp.dgradclip, lp.ggradclip) == (5, 0.7, 2, 1.0, 0.1)
    assert lp.stop is None and lp.fixed_critic_iter is None and not lp.graphed and lp.ema is s.ema and lp.evaluator is None
    assert lp.prefix == os.path.join(tmp_path, 'm') and lp.sample_every == 4 and lp.audio_every == 8
    assert s.sheets.samples == lp.L == 128          # one geometry for every sheet of the run
    assert lp.on_sample is s.sheets and s.sheets.every == 4 and s.sample_dir == lp.prefix + '-samples' == lp.sample_dir
    # 9 words in 10 train; the fixed sample words are those of the first held-out minibatch
    assert len(s.keys_train) == 9 and len(s.keys_valid) == 2 and set(s.keys_train) | set(s.keys_valid) == set(WORDS)
    cs, cl = lp._sample_words
    assert cs.shape == (4, 5) and np.array_equal(cs, s.first[5]) and np.array_equal(cl, s.first[6])
    assert all(''.join(chr(c) for c in row[:n]) in s.keys_valid for row, n in zip(cs, cl))
    assert (lp.dis_iter, lp.gen_iter) == (0, 0) and not os.path.exists(s.sample_dir)          # nothing has run
    # no sampling asked for: the loop gets none of it
    s0 = fit.build(fit.parse(SMALL + ['--outer', '1', '--device', 'cpu', '--dataset', store_path]))
    assert s0.loop.sample_every == 0 and s0.loop.on_sample is None and s0.ema is None and s0.loop.prefix is None
    assert len(s0.g.rnn) == 1 and isinstance(s0.opt_g, optim.RMSprop)


def test_build_refuses_a_store_the_loader_cannot_split(monkeypatch, tmp_path):
    _models(monkeypatch)
    p = os.path.join(tmp_path, 'six.npz')
    ingest.save_store(two_tone_store(WORDS[:6]), p)
    with pytest.raises(ValueError, match='at least 10 words'):
        fit.build(fit.parse(SMALL + ['--outer', '1', '--device', 'cpu', '--dataset', p]))


def test_loaditerations_restores_the_counters(monkeypatch, store_path, tmp_path):
    _models(monkeypatch)
    from audiogan_amd import checkpoint
    prefix = os.path.join(tmp_path, 'old', 'm')
    os.makedirs(os.path.dirname(prefix))
    argv = SMALL + ['--outer', '0', '--device', 'cpu', '--dataset', store_path]
    s = fit.build(fit.parse(argv))
    with torch.no_grad():
        for p in s.g.parameters():
            p.add_(0.125)
    checkpoint.save(prefix, 7, d=s.d, g=s.g, e_g=s.e_g, e_d=s.e_d, opt_d=s.opt_d, opt_g=s.opt_g,
                    extra=dict(dis_iter=21, gen_iter=7, baseline=0.5))
    want = [p.detach().clone() for p in s.g.parameters()]
    s2 = fit.build(fit.parse(argv + ['--modelnameload', prefix, '--loaditerations', '7', '--modelnamesave', os.path.join(tmp_path, 'new')]))
    extra = fit.resume(s2, prefix, 7)
    assert extra['gen_iter'] == 7 and (s2.loop.dis_iter, s2.loop.gen_iter, s2.loop.baseline) == (21, 7, 0.5)
    assert s2.loop.prefix == os.path.join(tmp_path, 'new')          # it saves where it was told to, not where it loaded
    assert all(torch.equal(p.detach(), q) for p, q in zip(s2.g.parameters(), want))


# ---- main, one pass on the kernel models -------------------------------------------------------------------------------------
def test_main_runs_a_pass_and_resumes(monkeypatch, store_path, tmp_path, capsys):
    _models(monkeypatch)
    prefix = os.path.join(tmp_path, 'run', 'm')
    rows = os.path.join(tmp_path, 'rows.jsonl')
    argv = SMALL + ['--device', 'cpu', '--dataset', store_path, '--modelnamesave', prefix, '--fixed-critic-iter', '2',
                    '--stop', 'never', '--sample-every', '1', '--sheet-every', '1', '--audio-every', '1', '--ema', '0.99',
                    '--checkpoint-every', '1', '--summary', rows, '--sheet-cols', '3', '--seed', '3']
    assert fit.main(argv + ['--outer', '1']) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (out['dis_iter'], out['gen_iter'], out['dis_iter_run'], out['gen_iter_run']) == (2, 1, 2, 1)
    assert out['summary']['kind'] == 'G' and out['summary']['iter'] == 1 and out['evaluation'] is None
    for role in ('dis', 'gen', 'eg', 'ed', 'opt', 'genema', 'egema'):          # the reference's names (audiogan.py:936-939)
        assert '%s-%s-%05d' % (prefix, role, 1) in out['files']
    names = {os.path.basename(p) for p in out['files']}
    assert {'m-run.json', 'real-sheet.png', 'sheet-1.png', 'sample-00001-0.wav', 'sample-00001-3.wav', 'rows.jsonl'} <= names
    assert all(os.path.exists(p) for p in out['files'])
    run = json.load(open(prefix + '-run.json'))
    assert run['framesize'] == 32 and run['outer'] == 1 and run['gstruct'] == [[17, 8, 16, 8], [9, 4, 16, 8]] and run['seed'] == 3
    geo = sheet.sheet_geometry(4, 128, cols=3)
    for name in ('real-sheet.png', 'sheet-1.png'):
        img = read_png(os.path.join(prefix + '-samples', name))
        assert img.shape == (geo['H'], geo['W'], 3) and geo['rows'] == 2
        assert (img[2:2 + 64, 2:3] != np.array(sheet.BG, dtype=np.uint8)).any()          # the first tile has an envelope
    kinds = [json.loads(line)['kind'] for line in open(rows)]
    assert kinds == ['D', 'D', 'G']          # one row per iteration
    # resume after pass 1, run pass 2: the counters a run of two passes ends at
    assert fit.main(argv + ['--outer', '1', '--loaditerations', '1']) == 0
    out2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (out2['dis_iter'], out2['gen_iter'], out2['dis_iter_run'], out2['gen_iter_run']) == (4, 2, 2, 1)
    assert '%s-gen-%05d' % (prefix, 2) in out2['files'] and '%s-gen-%05d' % (prefix, 1) not in out2['files']
    assert 'real-sheet.png' not in {os.path.basename(p) for p in out2['files']}          # written once, at iteration 0

"""``python -m audiogan_amd.fit`` on the GPU (-m gpu): ``fit.main`` on a synthetic store of two-tone words (eleven of them, four
clips each - the loader trains on 9 words in 10, so ten is the least a store may hold) at the small widths of the captured-loop
tests (tests/test_gpu_front_frames.py: frame 40, 320 samples, states 128 / 64), two passes eager and captured: checkpoints under
the reference's names, the two kinds of sample sheet at the geometry ``sheet_geometry`` predicts, one summary row per
iteration, the same checkpoint bytes from the same seed, a resumed run ending where the whole run ends, and ``synth.main`` on
what was written."""
import json
import os

import numpy as np
import pytest
import torch

from audiogan_amd import audio, fit, ingest, sheet, synth
from tests.test_fit import two_tone_store
from tests.test_sheet import read_png

pytestmark = pytest.mark.gpu

WIDTHS = ['--framesize', '40', '--noisesize', '8', '--gstatesize', '128', '--dstatesize', '64', '--embedsize', '8',
          '--charembedsize', '6', '--batchsize', '8', '--maxlen', '320', '--gstruct', '17,8,16,8;9,4,16,8', '--dstruct', '7,2,8;7,2,16']
RUN = ['--fixed-critic-iter', '2', '--stop', 'never', '--sample-every', '1', '--sheet-every', '1', '--ema', '0.99',
       '--checkpoint-every', '1', '--seed', '4']
ROLES = ('dis', 'gen', 'eg', 'ed', 'opt', 'genema', 'egema')


@pytest.fixture(scope='module')
def store_path(tmp_path_factory):
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    p = os.path.join(tmp_path_factory.mktemp('store'), 'words.npz')
    ingest.save_store(two_tone_store(clips=4, maxlen=320, seed=1), p)
    return p


def _main(capsys, store_path, folder, *extra):
    prefix = os.path.join(folder, 'm')
    argv = WIDTHS + RUN + ['--dataset', store_path, '--modelnamesave', prefix, '--summary', os.path.join(folder, 'rows.jsonl')]
    assert fit.main(argv + list(extra)) == 0
    return prefix, json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize('graphed', [False, True])
def test_two_passes_write_checkpoints_sheets_and_rows(capsys, store_path, tmp_path, graphed):
    prefix, out = _main(capsys, store_path, str(tmp_path), '--outer', '2', *(['--graphed'] if graphed else []))
    # (a captured loop's first pass runs two eager passes as its warm-up: real iterations, counted)
    dis, gen = (8, 4) if graphed else (4, 2)
    assert (out['dis_iter'], out['gen_iter'], out['dis_iter_run'], out['gen_iter_run']) == (dis, gen, dis, gen)
    for it in range(1, gen + 1):
        for role in ROLES:
            p = '%s-%s-%05d' % (prefix, role, it)
            assert os.path.exists(p) and p in out['files'], p
    geo = sheet.sheet_geometry(8, 320, cols=8)
    for name in ['real-sheet.png'] + ['sheet-%d.png' % it for it in range(1, gen + 1)]:
        img = read_png(os.path.join(prefix + '-samples', name))
        assert img.shape == (geo['H'], geo['W'], 3) == (2 + 64 + 129 + 2, 2 + 8 * 5, 3), name
        bg = np.array(sheet.BG, dtype=np.uint8)
        assert (img[:2] == bg).all() and (img[:, :2] == bg).all() and (img[2 + 64:2 + 193, 3:5] == bg).all()      # (one frame a clip)
        assert (img[2 + 64:2 + 193, 2] != bg).any(1).all(), name          # the first tile's one spectrogram column
        for b in range(8):          # every clip, real or sampled (the sampler draws its stops: ragged), has a first envelope column
            assert (img[2:2 + 64, 2 + 5 * b] != bg).any(1).all(), (name, b)
    rows = [json.loads(line) for line in open(os.path.join(tmp_path, 'rows.jsonl'))]
    assert len(rows) == dis + gen and sorted(r['iter'] for r in rows if r['kind'] == 'G') == list(range(1, gen + 1))
    assert sorted(r['iter'] for r in rows if r['kind'] == 'D') == list(range(1, dis + 1))
    assert out['summary'] == rows[-1] and all(np.isfinite(r['loss']) for r in rows if r['kind'] == 'D')
    assert json.load(open(prefix + '-run.json'))['graphed'] is graphed


def test_same_seed_same_checkpoint_bytes_and_a_resumed_run_ends_where_the_whole_run_ends(capsys, store_path, tmp_path):
    a, b, c = (str(tmp_path / n) for n in 'abc')
    pa, out_a = _main(capsys, store_path, a, '--outer', '2')
    pb, out_b = _main(capsys, store_path, b, '--outer', '2')
    for it in (1, 2):
        for role in ROLES:
            assert open('%s-%s-%05d' % (pa, role, it), 'rb').read() == open('%s-%s-%05d' % (pb, role, it), 'rb').read(), (role, it)
    assert open(os.path.join(pa + '-samples', 'sheet-2.png'), 'rb').read() == open(os.path.join(pb + '-samples', 'sheet-2.png'), 'rb').read()
    # pass 1, then a second process' worth: load iteration 1, run pass 2
    pc, out_1 = _main(capsys, store_path, c, '--outer', '1')
    assert (out_1['dis_iter'], out_1['gen_iter']) == (2, 1)
    pc, out_2 = _main(capsys, store_path, c, '--outer', '1', '--loaditerations', '1')
    assert (out_2['dis_iter'], out_2['gen_iter']) == (out_a['dis_iter'], out_a['gen_iter']) == (4, 2)
    assert (out_2['dis_iter_run'], out_2['gen_iter_run']) == (2, 1) and os.path.exists('%s-gen-%05d' % (pc, 2))


def test_synth_says_something_with_the_written_checkpoint(capsys, store_path, tmp_path):
    prefix, out = _main(capsys, store_path, str(tmp_path), '--outer', '1')
    wav = os.path.join(tmp_path, 'say.wav')
    assert synth.main(['--checkpoint', prefix, '--iteration', '1', '--text', 'alpha beta', '--out', wav, '--max-seconds', '0.04']) == 0
    data, sr = audio.read_wav(wav)
    assert sr == 16000 and data.dtype == np.int16 and data.shape[0] >= 2 * 2 * 40 and data.any()

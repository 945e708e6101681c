"""Activity detection on the CPU: the rule on hand-written flag patterns (``audio.activity_rule`` and the model of
ag_activity_segments, tests/activity_model.py), the mutants the checkers must reject, the model of ag_frame_power under the
GPU checkers, both launchers' refusals (host code, no GPU), ``audio.activity64`` on the burst inputs, and
``ingest.build_store(trim / split)``, ``write_cuts`` and the command-line tool on a byte-built tree.
-m gpu: tests/test_gpu_activity.py.  The bounds and where they come from: the module text of tests/activity_model.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from audiogan_amd import audio, ingest
from tests import activity_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fact', M.FACTS, ids=[f['name'] for f in M.FACTS])
def test_rule_facts(fact):
    """the hand-written expectation, ``activity_rule`` (run by run) and the model (frame by frame) agree"""
    segs, count, pmax = audio.activity_rule(np.array(fact['rows'], dtype=np.float32), fact['nf'], fact['lens'], fact['ratio'],
                                            fact['floor'], fact['min_gap'], fact['min_run'], fact['pad'], fact['win'], fact['hop'])
    if fact['want'][0] is None:
        assert segs == [None] and count.tolist() == [-1] and np.isnan(pmax[0])
    else:
        assert segs[0].dtype == np.int64 and segs[0].shape == (count[0], 2)
        assert [tuple(r) for r in segs[0].tolist()][:fact['K']] == fact['want'][0] and count.tolist() == fact['count']
        assert pmax[0] == max(fact['rows'][0])
    M.check_segments(M.activity_segments, [fact])


def test_rule_on_chunk_patterns_and_edge_rows():
    import audiogan_amd.kernels as K
    assert K.ACTIVITY_CHUNK == 1024
    M.check_segments(M.activity_segments, M.chunk_patterns(K.ACTIVITY_CHUNK))
    # nf = 0, a row of -0 only (pmax keeps the sign), an infinity past nf is not seen, one at nf - 1 is
    p = np.array([[1, 1, 1], [-0.0, -0.0, -0.0], [1, 1, np.inf], [1, 1, np.inf]], dtype=np.float32)
    segs, count, pmax = audio.activity_rule(p, [0, 3, 2, 3], [100] * 4, 0.5, 0.0, 1, 1, 0, 25, 10)
    assert count.tolist() == [0, 0, 1, -1] and segs[3] is None and segs[2].tolist() == [[0, 35]]
    assert pmax.view(np.int32).tolist()[:3] == [0, -2 ** 31, np.float32(1).view(np.int32)]
    case = dict(name='edge rows', rows=p.tolist(), nf=[0, 3, 2, 3], lens=[100] * 4, ratio=0.5, floor=0.0, min_gap=1, min_run=1, pad=0,
                win=25, hop=10, K=2)
    M.check_segments(M.activity_segments, [case])
    # the floor: a quiet row whose loudest frame lies under it has no active frame
    segs, count, _ = audio.activity_rule(np.full((1, 4), 1e-9, dtype=np.float32), [4], [100], 1e-4, 1e-8, 1, 1, 0, 25, 10)
    assert count.tolist() == [0] and segs[0].shape == (0, 2)


@pytest.mark.parametrize('mutant', M.MUTANTS)
def test_checkers_reject_mutants(mutant):
    """drop before close, >= for >, the pad not clipped, count capped at K: the checker over the facts must fail"""
    fn = lambda *a, **k: M.activity_segments(*a, mutate=mutant, **k)          # noqa: E731
    with pytest.raises(AssertionError):
        M.check_segments(fn, M.FACTS)


def test_parameters():
    q = audio.activity_params()
    assert (q['win'], q['hop'], q['min_gap'], q['min_run'], q['pad']) == (200, 80, 30, 5, 3)
    assert q['ratio'].dtype == np.float32 and q['ratio'] == np.float32(1e-4) and q['floor'] == np.float32(1e-8)
    q = audio.activity_params(16000, min_gap_ms=301.0, min_run_ms=10.0, pad_ms=0.0)
    assert (q['win'], q['hop'], q['min_gap'], q['min_run'], q['pad']) == (400, 160, 31, 1, 0)
    with pytest.raises(ValueError):
        audio.activity_params(8000, win_ms=5.0, hop_ms=10.0)
    with pytest.raises(ValueError):
        audio.activity_params(48000, win_ms=100.0)
    assert audio.frame_count(np.array([0, 1, 80, 81]), 80).tolist() == [0, 1, 1, 2]


# ------------------------------------------------------------------------------------------------------------------
# 2. the model of the power launch under the GPU checkers
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', M.SHAPES)
def test_power_model_against_float64(shape):
    import audiogan_amd.kernels as K
    tile = K.frame_power_tile(*shape)
    assert 1 <= tile <= K.FRAME_POWER_TILE_MAX
    worst = M.check_power_bound(M.frame_power, M.power_cases(*shape, tile) + M.far_cases(*shape))
    print('model, win %d hop %d: largest |p - p64| / bound %.4f' % (shape + (worst,)))
    M.check_power_integer(M.frame_power, M.power_cases(*shape, tile, integer=True))


def test_power_checkers_reject_a_wrong_window():
    """a frame one sample late, and a sample at or past a row's length read: both passes must fail"""
    late = lambda src, ln, win, hop, **k: M.frame_power(src, ln, win, hop, **dict(k, in_start=k['in_start'] + 1))          # noqa: E731
    past = lambda src, ln, win, hop, **k: M.frame_power(src, None, win, hop, **k)          # noqa: E731
    for fn in (late, past):
        with pytest.raises(AssertionError):
            M.check_power_integer(fn, M.power_cases(200, 80, 126, integer=True))
        with pytest.raises(AssertionError):
            M.check_power_bound(fn, M.power_cases(200, 80, 126))


# ------------------------------------------------------------------------------------------------------------------
# 3. the launchers
# ------------------------------------------------------------------------------------------------------------------
_HOST = ctypes.create_string_buffer(64 + 16)
PTR = (ctypes.addressof(_HOST) + 15) & ~15


def test_launchers_refuse_before_any_hip_call():
    """AG_ERR_ARG from host code, with no device in sight (the pointers are host memory: a launch would not survive them)"""
    import audiogan_amd.kernels as K
    from audiogan_amd import _lib
    p = ctypes.c_void_p(PTR)
    ok = dict(src=p, pitch=1000, lens=p, n_in=1000, in_start=0, win=200, hop=80, dst=p, ldd=13, f_start=0, n_frames=13, B=3)

    def power(**kw):
        a = dict(ok, **kw)
        return K.lib.ag_frame_power(a['src'], a['pitch'], a['lens'], a['n_in'], a['in_start'], a['win'], a['hop'], a['dst'], a['ldd'],
                                    a['f_start'], a['n_frames'], a['B'], None)
    for bad in (dict(hop=0), dict(hop=201), dict(win=4097, hop=80), dict(win=0, hop=0), dict(win=-200), dict(n_in=-1), dict(n_frames=-1),
                dict(B=-1), dict(in_start=-1), dict(f_start=-1), dict(pitch=-1), dict(ldd=-1), dict(src=None), dict(dst=None),
                dict(pitch=999), dict(ldd=12), dict(src=ctypes.c_void_p(PTR + 2)), dict(n_frames=1 << 41, ldd=1 << 41),
                dict(f_start=(1 << 40) + 1), dict(win=1, hop=1, n_frames=1 << 40, ldd=1 << 40, B=1 << 10)):
        assert power(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_frame_power'), bad
    assert power(B=0) == _lib.AG_OK and power(n_frames=0) == _lib.AG_OK
    assert power(B=0, src=None, dst=None) == _lib.AG_OK and power(n_frames=0, src=None, dst=None, lens=None) == _lib.AG_OK
    for args, want in (((200, 80), 1), ((1, 1), 1), ((4096, 4096), 1), ((4096, 1), 1), ((4097, 1), 0), ((80, 200), 0), ((5, 0), 0),
                       ((0, 0), 0), ((-4, -8), 0)):
        assert K.lib.ag_frame_power_ok(*args) == want and K.frame_power_ok(*args) == bool(want), args
        assert (K.frame_power_tile(*args) > 0) == bool(want), args
    assert K.frame_power_tile(200, 80) == 126          # 255 blocks of 40 samples: one round of the 256 threads

    ok = dict(power=p, pitch=98, nf=p, F=98, len=p, ratio=1e-4, floor=1e-8, min_gap=30, min_run=5, pad=3, win=200, hop=80, seg=p,
              K=4, count=p, pmax=p, B=2)

    def segs(**kw):
        a = dict(ok, **kw)
        return K.lib.ag_activity_segments(a['power'], a['pitch'], a['nf'], a['F'], a['len'], a['ratio'], a['floor'], a['min_gap'],
                                          a['min_run'], a['pad'], a['win'], a['hop'], a['seg'], a['K'], a['count'], a['pmax'], a['B'], None)
    for bad in (dict(min_gap=-1), dict(min_run=-1), dict(pad=-1), dict(K=-1), dict(F=-1), dict(B=65536), dict(B=-1), dict(hop=0),
                dict(hop=201), dict(win=4097), dict(power=None), dict(nf=None), dict(len=None), dict(seg=None), dict(count=None),
                dict(pmax=None), dict(pitch=97)):
        assert segs(**bad) == _lib.AG_ERR_ARG, bad
        assert K.lib.ag_last_error().startswith(b'ag_activity_segments'), bad
    assert segs(B=0) == _lib.AG_OK and segs(B=0, power=None, nf=None, len=None, seg=None, count=None, pmax=None) == _lib.AG_OK
    assert K.lib.ag_abi_version() == 13
    header = open(os.path.join(ROOT, 'include', 'audiogan_hip.h')).read()
    for sym in ('ag_frame_power_ok', 'ag_frame_power_tile', 'ag_frame_power', 'ag_activity_chunk', 'ag_activity_segments'):
        assert sym in _lib.SIGNATURES and 'int %s(' % sym in header
    assert 'preprocess-fisher.py:145-146' in header and 'preprocess.py:25-27' in header


# ------------------------------------------------------------------------------------------------------------------
# 4. activity64 on the burst inputs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', M.BURST_RATES)
def test_activity64_on_the_bursts(sr):
    y = M.burst_signal(sr)
    assert y.shape == (8000,) and M.margin(y) >= 1.5
    q = audio.activity_params()
    p = audio.frame_power64(y, 8000, q['win'], q['hop'])
    on = np.flatnonzero(p > max(p.max() * float(q['ratio']), float(q['floor'])))
    assert on[0] == 28 and on[-1] in (69, 70) and len(on) == on[-1] - 27          # (resampling smears the burst's end by a frame)
    got = audio.activity64(y)
    assert len(got) == 1 and got[0].tolist() == [[(28 - 3) * 80, (int(on[-1]) + 3) * 80 + 200]]
    assert audio.activity(y, device='cpu')[0].tolist() == got[0].tolist()
    # rows with lengths, a tensor source, a row with a NaN, an empty row
    rows = np.stack([y, np.roll(y, 800), y, y])
    rows[2, 5000] = np.nan
    got4 = audio.activity(torch.from_numpy(rows), lens=[8000, 8000, 8000, 0], device='cpu')
    assert got4[0].tolist() == got[0].tolist() and got4[1].tolist() == (got[0] + 800).tolist() and got4[2] is None
    assert got4[3].shape == (0, 2) and got4[3].dtype == np.int64
    assert audio.activity(rows, lens=[8000, 8000, 4000, 0], device='cpu')[2].tolist() == [[2000, 4000]]          # NaN past the length


# ------------------------------------------------------------------------------------------------------------------
# 5. build_store(trim / split), write_cuts, the tool
# ------------------------------------------------------------------------------------------------------------------
def test_build_store_trim_and_split(tmp_path):
    entries, facts = M.make_gate_tree(os.path.join(tmp_path, 'tree'))
    for y in facts['clips']:
        assert M.margin(y) >= 1.5
    assert [e[1] for e in entries] == ['alpha', 'beta', 'beta', 'gamma']
    store, report = ingest.build_store(entries, device='cpu', trim=True)
    M.check_gate_store(store, report, facts, 'trim')
    assert store['alpha'].shape == (1, 9560) and store['beta'].shape == (1, 3160)
    out = os.path.join(tmp_path, 'split.npz')
    store, report = ingest.build_store(entries, out_path=out, device='cpu', split=True)
    M.check_gate_store(store, report, facts, 'split')
    assert store['alpha'].shape == (2, 3160) and sorted(ingest.load_store(out)) == ['alpha', 'beta', 'gamma']
    both, rep2 = ingest.build_store(entries, device='cpu', trim=True, split=True)          # together: as split
    M.check_gate_store(both, rep2, facts, 'split')
    # 'too_long' applies to each resulting clip; the options reach audio.activity
    _, rep = ingest.build_store(entries, device='cpu', trim=True, maxlen=4000)
    assert rep['dropped']['too_long'] == [facts['paths']['two']] and rep['kept'] == dict(beta=1, gamma=1)
    _, rep = ingest.build_store(entries, device='cpu', split=True, maxlen=4000)
    assert rep['dropped']['too_long'] == [] and rep['kept'] == dict(alpha=2, beta=1, gamma=1)
    store, rep = ingest.build_store(entries, device='cpu', split=True, activity=dict(min_gap_ms=600.0, pad_ms=0.0))
    assert store['alpha'].shape == (1, 11320 - 2240) and rep['segments'][facts['paths']['two']][0] == [(2240, 11320)]
    store, rep = ingest.build_store(entries, device='cpu', split=True, activity=dict(min_run_ms=20.0))          # the click passes
    assert rep['segments'][facts['paths']['click']] == [[(2000, 5160), ((119 - 3) * 80, (120 + 3) * 80 + 200)]]
    # an unreadable file, and a clip that holds a NaN
    bad = os.path.join(tmp_path, 'tree', 'beta', 'broken.wav')
    with open(bad, 'wb') as f:
        f.write(b'RIFX' + bytes(40))
    nan = np.zeros(4000, dtype=np.float32)
    nan[100] = np.nan
    from tests.ingest_model import wav_bytes
    with open(os.path.join(tmp_path, 'tree', 'beta', 'nan.wav'), 'wb') as f:
        f.write(wav_bytes(nan.astype('<f4').tobytes(), 8000, 1, 32, tag=3))
    _, rep = ingest.build_store(list(ingest.scan_tree(os.path.join(tmp_path, 'tree'))), device='cpu', trim=True)
    assert sorted(os.path.basename(p) for p in rep['dropped']['unreadable']) == ['broken.wav', 'nan.wav']


def test_options_off_change_nothing(tmp_path, monkeypatch):
    from tests.ingest_model import TREE_MAXLEN, make_tree
    entries, _ = make_tree(os.path.join(tmp_path, 'tree'))
    monkeypatch.setattr(audio, 'activity', lambda *a, **k: pytest.fail('audio.activity called with the options off'))
    a, ra = ingest.build_store(entries, maxlen=TREE_MAXLEN, device='cpu')
    b, rb = ingest.build_store(entries, maxlen=TREE_MAXLEN, device='cpu', trim=False, split=False, activity=dict(top_db=30.0))
    assert list(a) == list(b) and all(np.array_equal(a[w].view(np.int32), b[w].view(np.int32)) for w in a)
    assert ra == rb and sorted(ra) == ['dropped', 'files', 'kept', 'seconds_in', 'seconds_out']


def test_cuts_then_manifest_give_the_split_store(tmp_path, capsys):
    """--split --cuts-out, then --manifest on its output: the same store bit for bit; --files with and without --word"""
    root = os.path.join(tmp_path, 'tree')
    entries, facts = M.make_gate_tree(root)
    direct, cuts, again = (os.path.join(tmp_path, n) for n in ('direct.npz', 'cuts.tsv', 'again.npz'))
    assert ingest.main(['--tree', root, '--out', direct, '--device', 'cpu', '--split', '--cuts-out', cuts]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep['kept'] == dict(alpha=2, beta=1) and rep['dropped'] == dict(silent=1, too_long=0, unreadable=0)
    assert abs(rep['seconds_trimmed'] - (16000 - 2 * 3160 + 12000 - 3160) / 8000.0) < 1e-9
    lines = [ln.rstrip('\n').split('\t') for ln in open(cuts) if not ln.startswith('#')]
    assert [(os.path.basename(c[0]), c[1]) for c in lines] == [('two.wav', 'alpha'), ('two.wav', 'alpha'), ('click.wav', 'beta')]
    assert [c[2:] for c in lines[:2]] == [['%.6f' % ((s + 0.5) / 8000) for s in r] for r in ((2000, 5160), (8400, 11560))]
    got = ingest.read_manifest(cuts)
    assert [(int(s * 8000), int(e * 8000)) for _, _, s, e in got] == [(2000, 5160), (8400, 11560), (2000, 5160)]
    assert ingest.main(['--manifest', cuts, '--out', again, '--device', 'cpu']) == 0
    capsys.readouterr()
    a, b = ingest.load_store(direct), ingest.load_store(again)
    assert list(a) == list(b) == ['alpha', 'beta']
    assert all(a[w].shape == b[w].shape and np.array_equal(a[w].view(np.int32), b[w].view(np.int32)) for w in a)
    # every sample index survives the text: the half sample absorbs the rounding
    rep = dict(segments={'x.wav': [[(s, s + 1) for s in list(range(0, 4000, 7)) + [10 ** 6 + 1, 2 ** 31 + 3]]]})
    n = ingest.write_cuts(rep, [('x.wav', 'w', None, None)], cuts)
    back = ingest.read_manifest(cuts)
    assert n == len(back) and [int(s * 8000) for _, _, s, _ in back] == [s for s, _ in rep['segments']['x.wav'][0]]
    # --files: the segment-then-label workflow (the default label '?'), and a given --word with --trim
    assert ingest.main(['--files', facts['paths']['two'], '--out', again, '--device', 'cpu', '--split', '--cuts-out', cuts]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['kept'] == {'?': 2}
    assert [e[1] for e in ingest.read_manifest(cuts)] == ['?', '?']
    assert ingest.main(['--files', facts['paths']['two'], facts['paths']['click'], '--word', 'yes', '--out', again, '--device', 'cpu',
                        '--trim', '--top-db', '40', '--floor-db', '-80', '--min-gap-ms', '300', '--min-run-ms', '50', '--pad-ms',
                        '30']) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['kept'] == dict(yes=2)
    assert ingest.load_store(again)['yes'].shape == (2, 9560)
    with pytest.raises(SystemExit):
        ingest.main(['--tree', root, '--out', again, '--cuts-out', cuts])
    capsys.readouterr()

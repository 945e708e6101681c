"""Activity detection on the GPU (-m gpu): ag_frame_power under the checkers of tests/activity_model.py (the bound pass against
float64, the integer pass bit for bit, NaN-filled guarded destinations), chunks against the whole, starts past 2^33;
ag_activity_segments against ``audio.activity_rule`` on the CPU file's facts and on patterns that cross the launch's chunk;
``audio.activity`` on the device against ``activity64``; ``ingest.build_store(device='cuda', trim / split)`` on the CPU test's
tree.  The bounds: the module text of tests/activity_model.py; every ratio is printed before it is asserted
(tools/prof_activity.py writes them to profiles/activity_fuzz.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from audiogan_amd import audio, ingest
from tests import activity_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


@pytest.mark.parametrize('shape', M.SHAPES)
def test_power_bound_pass(K, shape):
    """three launches of three ragged rows (0, 1, win - 1, win, win + 1 samples; one, zero and minus one frame around the
    launch's tile), a row pitch above the width, noise of amplitude 1e-3 and a full-scale square wave"""
    tile = K.frame_power_tile(*shape)
    worst = M.check_power_bound(K.frame_power, M.power_cases(*shape, tile), on=_cuda)
    print('ag_frame_power win %d hop %d (tile %d): largest |p - p64| / bound %.4f' % (shape + (tile, worst)))
    assert K.lib.ag_last_kernel().decode() == 'frame_power_kernel'


@pytest.mark.parametrize('shape', M.SHAPES)
def test_power_integer_pass(K, shape):
    M.check_power_integer(K.frame_power, M.power_cases(*shape, K.frame_power_tile(*shape), integer=True), on=_cuda)


def test_power_alignments(K):
    """rows that start 0 .. 3 floats off a 16-byte boundary, exact in integers: the aligned groups of the staging shift"""
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randint(-64, 65, size=2 * 1003 + 8).astype(np.float32)).cuda()
    for off in range(4):
        src = x[off:off + 2 * 1003].view(2, 1003)[:, :1000]
        p = K.frame_power(src, None, 200, 80).cpu().numpy()
        for b in range(2):
            want = np.rint(M.power64(src[b].cpu().numpy(), 1000, 200, 80, 13) * 200).astype(np.float32) * (np.float32(1) / np.float32(200))
            assert np.array_equal(p[b], want), (off, b)


def test_chunks_have_the_bits_of_the_whole(K):
    """one row of 40 000 samples at once, and in chunks of 37 frames, each a row of its own holding just the samples its frames
    read, with in_start / f_start"""
    x = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, (1, 40000)).astype(np.float32)).cuda()
    for win, hop in ((200, 80), (256, 64), (33, 32)):
        whole = K.frame_power(x, None, win, hop)
        F = (40000 + hop - 1) // hop
        assert tuple(whole.shape) == (1, F)
        parts = torch.full_like(whole, float('nan'))
        for f0 in range(0, F, 37):
            f1 = min(F, f0 + 37)
            lo, hi = f0 * hop, min(40000, (f1 - 1) * hop + win)
            K.frame_power(x[:, lo:hi].contiguous(), None, win, hop, dst=parts[:, f0:f1], in_start=lo, f_start=f0)
        assert torch.equal(whole.view(torch.int32), parts.view(torch.int32)), (win, hop)


def test_far_start(K):
    """in_start and f_start hop past 2^33 on rows of a few hundred samples, against float64 with Python integers"""
    table = M.far_cases(200, 80) + M.far_cases(256, 64)
    assert all(c['in_start'] > (1 << 33) and c['f_start'] * c['hop'] > (1 << 33) for c in table)
    M.check_power_bound(K.frame_power, table, on=_cuda)


def test_segments_facts_and_chunk_patterns(K):
    """the CPU file's facts; a gap and a run that straddle the chunk boundary; the alternating pattern over two chunks and a
    bit with K below, equal to and above the count: seg, count and pmax equal activity_rule, untouched entries hold -1"""
    M.check_segments(K.activity_segments, M.FACTS, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == 'activity_segments_kernel'
    M.check_segments(K.activity_segments, M.chunk_patterns(K.ACTIVITY_CHUNK), on=_cuda)
    p = [[1, 1, 1], [-0.0, -0.0, -0.0], [1, 1, float('inf')], [1, 1, float('inf')]]
    M.check_segments(K.activity_segments, [dict(name='edge rows', rows=p, nf=[0, 3, 2, 3], lens=[100] * 4, ratio=0.5, floor=0.0,
                                                min_gap=1, min_run=1, pad=0, win=25, hop=10, K=2)], on=_cuda)
    # K = 0 writes no segment; a fresh seg holds -1 where nothing is written
    seg, count, pmax = K.activity_segments(torch.tensor([[1.0, 0.0, 1.0]]).cuda(), torch.tensor([3], dtype=torch.int32).cuda(),
                                           torch.tensor([100]).cuda(), 0.5, 0.0, 1, 1, 0, 10, 10, K=0)
    assert tuple(seg.shape) == (1, 0, 2) and count.tolist() == [2] and pmax.tolist() == [1.0]
    seg, count, _ = K.activity_segments(torch.tensor([[1.0, 0.0, 1.0]]).cuda(), torch.tensor([3], dtype=torch.int32).cuda(),
                                        torch.tensor([100]).cuda(), 0.5, 0.0, 1, 1, 0, 10, 10, K=3)
    assert seg.tolist() == [[[0, 10], [20, 30], [-1, -1]]] and count.tolist() == [2]


def test_a_long_row_of_random_runs(K):
    """10^5 frames of random runs and gaps of 1 .. 60 frames, three rows with different rules' parameters in turn"""
    rs = np.random.RandomState(8)
    F = 100000
    rows = []
    for _ in range(3):
        edges = np.cumsum(rs.randint(1, 61, size=F // 20))
        edges = edges[edges < F]
        flag = np.zeros(F, dtype=np.float32)
        for a, e in zip(edges[0::2], edges[1::2]):
            flag[a:e] = 1.0
        rows.append((flag * rs.uniform(0.6, 1.0, F)).astype(np.float32).tolist())
    for min_gap, min_run, pad in ((30, 5, 3), (0, 0, 0), (7, 40, 10)):
        M.check_segments(K.activity_segments, [dict(name='long', rows=rows, nf=[F, F - 1, F // 2], lens=[F * 80 + 120, F * 80, F * 40],
                                                    ratio=0.5, floor=0.0, min_gap=min_gap, min_run=min_run, pad=pad, win=200, hop=80,
                                                    K=4096)], on=_cuda)


@pytest.mark.parametrize('sr', M.BURST_RATES)
def test_activity_on_the_device_against_activity64(K, sr):
    y = M.burst_signal(sr)
    assert M.margin(y) >= 1.5          # no frame within fp32 reach of the threshold: the two paths must agree
    want = audio.activity64(y)
    assert len(want[0]) == 1
    got = audio.activity(torch.from_numpy(y).cuda())
    assert got[0].dtype == np.int64 and got[0].tolist() == want[0].tolist()
    host = audio.activity(y, device='cuda', chunk=1000)          # a host source, uploaded in windows of 1000 samples
    assert host[0].tolist() == want[0].tolist()
    # more runs than max_segments: the segment launch runs once more with K = the largest count
    short = dict(min_gap_ms=10.0, min_run_ms=10.0, pad_ms=0.0, win_ms=10.0)
    z = np.zeros(8000, dtype=np.float32)
    z[::160] = 0.5          # one frame in two holds a click
    rows = np.stack([z, np.roll(z, 80)])
    got = audio.activity(rows, device='cuda', max_segments=4, **short)
    want = audio.activity64(rows, **short)
    assert len(want[0]) == len(want[1]) == 50 and [g.tolist() for g in got] == [w.tolist() for w in want]


def test_build_store_on_the_device(K, tmp_path):
    """the CPU test's tree through build_store(device='cuda', trim / split): the segments and the stores of the CPU run"""
    entries, facts = M.make_gate_tree(os.path.join(tmp_path, 'tree'))
    for y in facts['clips']:
        assert M.margin(y) >= 1.5
    for mode in ('trim', 'split'):
        store, report = ingest.build_store(entries, device='cuda', **{mode: True})
        M.check_gate_store(store, report, facts, mode)
        host, rep = ingest.build_store(entries, device='cpu', **{mode: True})
        assert rep['segments'] == report['segments'] and list(host) == list(store)
        assert all(np.array_equal(host[w].view(np.int32), store[w].view(np.int32)) for w in host)


def test_the_tool_on_the_device(K, tmp_path):
    """``python -m audiogan_amd.ingest --device cuda --split --cuts-out`` in a process of its own (the package, not a test
    module, decides there in which order torch and the library are loaded): the store of the call in this process"""
    root = os.path.join(tmp_path, 'tree')
    entries, facts = M.make_gate_tree(root)
    out, cuts = os.path.join(tmp_path, 'cli.npz'), os.path.join(tmp_path, 'cuts.tsv')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'audiogan_amd.ingest', '--tree', root, '--out', out, '--device', 'cuda', '--split',
                        '--cuts-out', cuts], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep['kept'] == dict(alpha=2, beta=1) and rep['dropped'] == dict(silent=1, too_long=0, unreadable=0)
    want, _ = ingest.build_store(entries[:3], device='cuda', split=True)
    got = ingest.load_store(out)
    assert list(got) == list(want) and all(np.array_equal(got[w].view(np.int32), want[w].view(np.int32)) for w in want)
    assert [(int(s * 8000), int(e * 8000)) for _, _, s, e in ingest.read_manifest(cuts)] == [(2000, 5160), (8400, 11560), (2000, 5160)]


def test_wrappers_bad_arguments_and_profiler(K):
    x = torch.zeros(2, 1000, device='cuda')
    with pytest.raises(RuntimeError):
        K.frame_power(x.cpu(), None, 200, 80)
    with pytest.raises(TypeError):
        K.frame_power(x.double(), None, 200, 80)
    with pytest.raises(TypeError):
        K.frame_power(x, torch.zeros(2, dtype=torch.int32, device='cuda'), 200, 80)
    with pytest.raises(ValueError):
        K.frame_power(x, None, 80, 200)
    p = K.frame_power(x, None, 200, 80, n_frames=0)
    assert tuple(p.shape) == (2, 0)
    K.Profiler.start()
    try:
        p = K.frame_power(x, None, 200, 80)
        K.activity_segments(p, torch.full((2,), 13, dtype=torch.int32, device='cuda'), torch.full((2,), 1000, device='cuda'),
                            1e-4, 1e-8, 30, 5, 3, 200, 80)
    finally:
        rec = K.Profiler.stop()
    assert sorted(rec) == ['activity_segments_kernel', 'frame_power_kernel'] and all(r['n'] == 1 for r in rec.values())

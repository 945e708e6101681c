"""Word cuts by template alignment on the GPU (-m gpu): kernels.dtw_align / ag_dtw_align under the checkers of
tests/dtwalign_model.py - equal to align.path64 on integer inputs at every edge of the launch (the wave edge, the 16-column
packing word, counts below capacity, the 1024 x 1024 limit), on real inputs bit-equal totals to kernels.dtw_cost and a
returned path within the recursion's bound of the optimum - then untouched memory, determinism, a side stream, and
align.align_utterances / the tool on the synthetic utterances of tests/test_dtwalign.py.

Outputs are NaN / -1 filled between guard words; the inputs hold NaN past the counts and outside columns 1..12, so a read of
either shows.  Each test prints what it measured (pytest -s; profiles/dtw_align_fuzz.txt)."""
import os

import numpy as np
import pytest
import torch

from audiogan_amd import align, ingest
from tests import dtwalign_model as M
from tests import test_dtwalign as TD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_integer_pass_at_every_edge(K):
    """rows 1, 2, 63, 64, 65, 129 x columns 1, 15, 16, 17, 33 at capacities 132 x 36, the all-equal pairs, the clamped
    counts: total, lo, hi EQUAL to path64's"""
    M.check_exact(K.dtw_align, M.GRID, 'integer', on=_cuda)
    assert K.lib.ag_last_kernel().decode() == 'dtw_align_kernel'
    M.check_exact(K.dtw_align, M.EQUAL, 'equal', on=_cuda)
    M.check_exact(K.dtw_align, M.CLAMP, 'integer', on=_cuda)
    M.check_exact(K.dtw_align, M.SMALL, 'integer', on=_cuda)
    # counts of None are the capacities
    ca, na, cb, nb, _ = M.make_case(dict(pairs=((34, 21), (34, 21)), Fa=34, Fb=21), 'integer', seed=4)
    total, lo, hi = M.run_guarded(K.dtw_align, ca, None, cb, None, ((34, 21), (34, 21)), on=_cuda)
    for b in range(2):
        want = align.path64(ca[b].numpy(), 34, cb[b].numpy(), 21)
        assert float(total[b]) == want[0] and np.array_equal(lo[b].numpy(), want[1]) and np.array_equal(hi[b].numpy(), want[2])


def test_the_limits(K):
    """one pair of 1024 x 1024 frames: integer inputs EQUAL to path64; real inputs bit-equal to dtw_cost and within the bound"""
    M.check_exact(K.dtw_align, M.LIMIT, 'integer', on=_cuda)
    ratio = M.check_real(K.dtw_align, M.LIMIT, on=_cuda, cost_fn=K.dtw_cost)
    print('dtw_align 1024 x 1024, real pass: (cost of the returned path - D64) / bound %.3e' % ratio)


def test_real_pass(K):
    """randn cepstra at every edge: the total bit-equal to kernels.dtw_cost on the same tensors, the path facts, and the
    float64 cost of the RETURNED path within align_model.dtw_real_bound of path64's optimum"""
    worst = 0.0
    for case in (M.GRID, M.SMALL, M.CLAMP):
        worst = max(worst, M.check_real(K.dtw_align, case, on=_cuda, cost_fn=K.dtw_cost))
    print('dtw_align real pass: largest (cost of the returned path - D64) / bound %.3e' % worst)


def test_determinism_workspace_and_side_stream(K):
    """two launches give the same bits; a caller's workspace (dirty, exactly the size asked for) changes nothing; one byte
    less is refused; a launch on a side stream gives the same bits"""
    ca, na, cb, nb, counts = M.make_case(M.GRID, 'real', seed=7)
    first = M.run_guarded(K.dtw_align, ca, na, cb, nb, counts, on=_cuda)
    again = M.run_guarded(K.dtw_align, ca, na, cb, nb, counts, on=_cuda)
    need = len(counts) * K.dtw_align_ws(M.GRID['Fa'], M.GRID['Fb'])
    assert need == len(counts) * 132 * 3 * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda')
    own = M.run_guarded(K.dtw_align, ca, na, cb, nb, counts, on=_cuda, workspace=ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = M.run_guarded(K.dtw_align, ca, na, cb, nb, counts, on=_cuda)
    s.synchronize()
    for got in (again, own, side):
        for a, b in zip(first, got):
            assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match='workspace'):
        K.dtw_align(ca.cuda(), na.cuda(), cb.cuda(), nb.cuda(), workspace=ws[:need - 1])
    with pytest.raises(ValueError, match='1024'):
        K.dtw_align(torch.zeros(1, 1025, 16, device='cuda'), None, torch.zeros(1, 4, 16, device='cuda'), None)
    with pytest.raises(TypeError, match='nf_a'):
        K.dtw_align(ca.cuda(), na.cuda().long(), cb.cuda(), nb.cuda())
    torch.cuda.synchronize()


def test_align_utterances_on_the_device(K):
    """the synthetic utterances: cuts within the CPU test's tolerance of the true boundaries, and EXACTLY path64's cuts when
    path64 is fed the kernel's own cepstra"""
    waves, lens, transcripts, truth = M.utterances()
    templates = align.pick_templates(M.template_store(), list(M.WORDS), device='cuda')
    got = align.align_utterances(waves, lens, transcripts, templates, device='cuda')
    assert K.lib.ag_last_kernel().decode() in ('dtw_pairs_wave_kernel', 'dtw_pairs_wg_kernel')          # (the scores came last)
    worst = M.boundary_errors(got, truth)
    print('align_utterances on the device: largest boundary error %.3f frames (path64 on float64 cepstra %.3f, tolerance %.3f)'
          % (worst, M.PATH64_WORST, M.BOUNDARY_TOLERANCE))
    assert worst <= M.BOUNDARY_TOLERANCE
    host = align.align_utterances(waves, lens, transcripts, templates, device='cuda', host_path=True)
    assert [[c[:3] for c in r['cuts']] for r in got] == [[c[:3] for c in r['cuts']] for r in host]
    assert all(np.isfinite(c[3]) and c[3] > 0 for r in got for c in r['cuts'])
    # a batch of one utterance per launch gives the same cuts and scores
    one = align.align_utterances(waves, lens, transcripts, templates, device='cuda', batch=1)
    assert one == got


def test_the_tool_on_the_device(K, tmp_path, capsys):
    """python -m audiogan_amd.ingest --utterances on the device; --cuts-out, then --manifest: the same store bit for bit"""
    tsv, npz, truth = TD.write_utterance_files(tmp_path)
    _, _, transcripts, _ = M.utterances()
    out, cuts, back = (os.path.join(tmp_path, n) for n in ('words2.npz', 'cuts.tsv', 'back.npz'))
    assert ingest.main(['--utterances', tsv, '--templates', npz, '--out', out, '--cuts-out', cuts, '--device', 'cuda']) == 0
    assert ingest.main(['--manifest', cuts, '--out', back, '--device', 'cuda']) == 0
    capsys.readouterr()
    a, b = ingest.load_store(out), ingest.load_store(back)
    assert list(a) == list(b) and all(np.array_equal(a[w], b[w]) for w in a)
    utts = ingest.read_utterances(tsv)
    templates = align.pick_templates(ingest.load_store(npz), list(M.WORDS), device='cuda')
    _, report = ingest.align_store(utts, templates, device='cuda')
    worst = TD.check_cuts_against_truth(report, truth, transcripts)
    print('ingest --utterances on the device: largest boundary error %.3f frames' % worst)

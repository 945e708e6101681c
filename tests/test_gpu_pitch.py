"""Pitch measures of the held-out evaluation on the GPU (-m gpu): kernels.pitch_frames / ag_pitch_frames and
kernels.pitch_path_accum / ag_pitch_path_accum on every case of the tables of tests/pitch_model.py, in the integer pass bit for
bit and in the real pass under the bound rule against audio.pitch64 / evaluate.pitch_path_sums64; the kernel names; a side
stream; evaluate.pitch_distance against the float64 path; Evaluator(aligned=True, pitch=True) on the tiny networks; a
training loop that evaluates with it.

Outputs are NaN / sentinel filled between guard elements; the inputs hold NaN past the lengths and the counts, so a read of
either shows; every case runs twice for identical bits.  The measured GPU-to-floor ratios are printed (profiles/pitch_fuzz.txt
keeps a run's)."""
import numpy as np
import pytest
import torch

from tests import pitch_model as M
from tests import test_evaluate as TE
from tests import test_pitch as TC


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


def _name(K):
    return lambda: K.lib.ag_last_kernel().decode()


# ------------------------------------------------------------------------------------------------------------------
# pitch_frames
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(M.FRAME_CASES))
def test_pitch_frames_integer_pass(K, name):
    TC.run_case(K.pitch_frames, name, 'integer', on=_cuda, kernel_name=_name(K))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(M.FRAME_CASES))
def test_pitch_frames_real_pass(K, name):
    r = TC.run_case(K.pitch_frames, name, 'real', on=_cuda, kernel_name=_name(K))
    print('pitch_frames %-14s GPU error / floor: phi %.3f  power %.3f' % (name, r['phi'], r['power']))


@pytest.mark.gpu
@pytest.mark.parametrize('which', M.SPECIAL)
def test_pitch_frames_special_clips(K, which):
    TC.run_special(K.pitch_frames, which, on=_cuda, kernel_name=_name(K))


@pytest.mark.gpu
def test_pitch_frames_on_the_tones(K):
    r = TC.run_tones(K.pitch_frames, on=_cuda, kernel_name=_name(K))
    print('pitch_frames tones          GPU error / floor: phi %.3f  power %.3f' % (r['phi'], r['power']))


@pytest.mark.gpu
def test_a_frames_bits_do_not_depend_on_its_tile_or_on_the_staging(K):
    """the same samples displaced by 8 and by 9 frames (another tile, another wave), and through the scalar staging"""
    x = M.harmonic(133.0, 2048, seed=4)
    base, _ = M.run_frames(K.pitch_frames, x[None, :], None, on=_cuda, kernel_name=_name(K))
    for shift in (8, 9):
        rows = np.concatenate([np.zeros(shift * 128, dtype=np.float32), x])[None, :].copy()
        out, _ = M.run_frames(K.pitch_frames, rows, None, on=_cuda)
        for k in ('nccf', 'peak', 'lag'):
            assert np.array_equal(out[k][0, shift:].view(np.int32), base[k][0].view(np.int32)), (shift, k)
    out, _ = M.run_frames(K.pitch_frames, x[None, :], None, on=_cuda, off=3, staging='scalar', kernel_name=_name(K))
    for k in ('nccf', 'peak', 'lag'):
        assert np.array_equal(out[k].view(np.int32), base[k].view(np.int32)), k


@pytest.mark.gpu
def test_pitch_frames_on_a_side_stream(K):
    rows, _ = M.case_rows('tile_plus_one', 'real')
    lens = M.FRAME_CASES['tile_plus_one']['lens']
    base, _ = M.run_frames(K.pitch_frames, rows, lens, on=_cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, _ = M.run_frames(K.pitch_frames, rows, lens, on=_cuda)
    side.synchronize()
    for k in ('nccf', 'peak', 'lag', 'nframes'):
        assert np.array_equal(out[k].view(np.int32), base[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------------------------------
# pitch_path_accum
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind_pass', ['integer', 'real'])
@pytest.mark.parametrize('name', sorted(M.PATH_CASES))
def test_pitch_path_accum(K, name, kind_pass):
    r = TC.run_path_case(K.pitch_path_accum, name, kind_pass, on=_cuda)
    assert K.lib.ag_last_kernel().decode() == 'pitch_path_accum_kernel'
    if kind_pass == 'real':
        print('pitch_path_accum %-10s GPU error / floor: sum d^2 %.3f' % (name, r))


@pytest.mark.gpu
def test_pitch_path_accum_gross_threshold_and_side_stream(K):
    TC.run_gross_edge(K.pitch_path_accum, on=_cuda)
    case = M.path_case('diagonal', 'real')
    base = M.run_path(K.pitch_path_accum, case, on=_cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = M.run_path(K.pitch_path_accum, case, on=_cuda)
    side.synchronize()
    assert np.array_equal(got, base)


# ------------------------------------------------------------------------------------------------------------------
# higher levels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pitch_distance_against_the_float64_path(K):
    from audiogan_amd.evaluate import aligned_distance, pitch_distance
    a, b = M.property_pair()
    want, _ = M.pitch_distance64(a, b)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = pitch_distance(ta, None, tb, None)
    mcd = aligned_distance(ta, None, tb, None).cpu().numpy()
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (2,) for v in got.values())
    TC.check_property({k: v.cpu() for k, v in got.items()}, mcd)
    # the device's fp32 cepstra may take another path of (nearly) the same cost than float64's: the counts may move by a
    # few cells, the F0 error by a fraction of the tolerance the property itself is asserted at
    for k in range(2):
        assert abs(float(got['cells'][k]) - float(want['cells'][k])) <= 4
        assert abs(float(got['f0_rmse_cents'][k]) - float(want['f0_rmse_cents'][k])) <= 0.5 * TC.PROPERTY_TOLERANCE_CENTS
    assert got['vuv_err'].tolist() == want['vuv_err'].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        pitch_distance(ta, None, torch.zeros(2, 131329, device='cuda'), None)


@pytest.mark.gpu
def test_pitch_run_gpu(K, tmp_path):
    import audiogan_amd as A
    K.lstm_persist_status(reset=True)
    s = TE._setup(A, torch.device('cuda'), 'toy_gpu', tmp_path, 8)
    TC.run_evaluator_checks(s)
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0


@pytest.mark.gpu
def test_eager_loop_with_pitch_evaluator_changes_no_training_bit(K, tmp_path):
    """an eager TrainLoop of 2 passes at toy_gpu with Evaluator(aligned, pitch) against one without an evaluator: every
    parameter and the CUDA generator state equal"""
    import audiogan_amd as A
    dev = torch.device('cuda')
    K.lstm_persist_status(reset=True)
    got = []
    for evaluating in (False, True):
        s = TE._setup(A, dev, 'toy_gpu', tmp_path, 8)
        torch.cuda.manual_seed(17)
        kw = dict(evaluator=TE._evaluator(s, aligned=True, pitch=True), eval_every=1) if evaluating else {}
        lp = s.mk(fixed_critic_iter=2, gencatchup=1, stop='never', checkpoint_every=0, check=False, host=False, **kw)
        for _ in range(2):
            lp.outer()
        if evaluating:
            assert len(lp.eval_log) == 2 and all(0 <= r['vuv_err'] <= 1 and 'f0_rmse_cents' in r for r in lp.eval_log)
        got.append(([p.detach().clone() for m in s.mods for p in m.parameters()], torch.cuda.get_rng_state()))
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[0][1], got[1][1])
    torch.cuda.synchronize()
    assert K.lstm_persist_status() == 0

"""Sample sheets on the GPU (-m gpu): ag_sheet_render under the checker of tests/sheet_model.py - byte for byte against the
pixel-by-pixel model on given power / wave tensors, NaN and large values in all padding, guard bytes around an image at every
byte alignment, two runs, a side stream - and ``sheet.render`` against ``sheet.render_host`` fed the device's own power, with a
``lens`` tensor that never leaves the device.  Every comparison is byte equality."""
import os

import numpy as np
import pytest
import torch

from audiogan_amd import sheet
from tests import sheet_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import audiogan_amd.kernels as K_
    return K_


def _cuda(t):
    return t.cuda()


@pytest.mark.parametrize('pad', M.PADS)
def test_launch_against_the_model_over_the_table(K, pad):
    """B 1, 3, 9 at 4 across; L 8, 256, 384, 1000 and one of two column tiles; lens 0, 1, 255, 256, L and above L; no lens;
    frame counts of 0, below 0 and above F; every byte alignment of the image; guards intact (the checker asserts them)"""
    for case in M.cases():
        first = M.run(K.sheet_render, case, pad, on=_cuda)
        assert K.lib.ag_last_kernel().decode() == 'sheet_render_kernel'
        again = M.run(K.sheet_render, case, pad, on=_cuda)
        assert torch.equal(first, again), case.name


def test_launch_on_a_side_stream(K):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name in ('nine_384', 'two_tiles', 'frame_counts'):
            M.run(K.sheet_render, [c for c in M.cases() if c.name == name][0], 'big', on=_cuda)
    side.synchronize()


def _clips(B, L, lens, seed, extra=0):
    rng = np.random.RandomState(seed)
    t = np.arange(L + extra)
    wave = np.stack([0.6 * np.sin(2 * np.pi * (200.0 + 310.0 * b) * t / 8000.0) * np.exp(-t / (300.0 + 90.0 * b)) +
                     0.02 * rng.standard_normal(L + extra) for b in range(B)]).astype(np.float32)
    for b, n in enumerate(lens):
        wave[b, min(max(n, 0), L):] = np.nan          # never read, by either launch
    return wave


@pytest.mark.parametrize('B,L,lens', [
    (1, 8, [8]),
    (3, 256, [0, 1, 255]),
    (9, 384, [0, 1, 255, 256, 384, 999, 257, 383, 128]),
    (3, 1000, [1000, 640, 1]),
    (2, 4400, [4400, 4099]),
])
def test_render_is_render_host_on_the_devices_power(K, B, L, lens):
    wave_h = _clips(B, L, lens, seed=B + L, extra=3)
    wave = torch.from_numpy(wave_h).cuda()[:, :L]          # a row pitch of L + 3
    lens_d = torch.tensor(lens, dtype=torch.int64).cuda()
    F = K.lt_frames(L)
    power = torch.full((B, F, 129), float('nan')).cuda()
    nframes = torch.zeros(B, dtype=torch.int32).cuda()
    opts = dict(cols=4, Hw=12, gutter=2)
    img = sheet.render(wave, lens_d, power=power, nframes=nframes, **opts)
    geo = sheet.sheet_geometry(B, L, **opts)
    assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (geo['H'], geo['W'], 3)
    assert nframes.cpu().tolist() == [K.lt_frames(min(max(n, 0), L)) for n in lens]
    want = sheet.render_host(wave_h[:, :L], np.array(lens), power.cpu().numpy(), nframes.cpu().numpy(), **opts)
    assert np.array_equal(img.cpu().numpy(), want)
    # into a caller's image, twice: equal bytes
    out = torch.zeros(geo['H'], geo['W'], 3, dtype=torch.uint8).cuda()
    assert sheet.render(wave, lens_d, out=out, **opts) is out and torch.equal(out, img)


def test_a_lens_tensor_that_stays_on_the_device(K, monkeypatch):
    """the lengths come out of device arithmetic and are never read: any host read of a tensor between the two launches raises"""
    B, L = 5, 640
    wave_h = _clips(B, L, [L] * B, seed=2)
    wave = torch.from_numpy(wave_h).cuda()
    lens_d = (torch.arange(B, device='cuda') * 160).long()          # 0, 160, .. 640
    opts = dict(cols=4, Hw=9, gutter=1)
    sheet.render(wave, lens_d, **opts)          # (tables uploaded, buffers warm)
    torch.cuda.synchronize()

    def no_read(*a, **k):
        raise AssertionError('a host read inside sheet.render')
    with monkeypatch.context() as m:
        for name in ('cpu', 'item', 'tolist', 'numpy'):
            m.setattr(torch.Tensor, name, no_read)
        img = sheet.render(wave, lens_d, **opts)
    want = sheet.render_host(wave_h, np.arange(B) * 160, *[t.cpu().numpy() for t in _power(K, wave, lens_d)], **opts)
    assert np.array_equal(img.cpu().numpy(), want)
    geo = sheet.sheet_geometry(B, L, **opts)
    tile0 = img[1:1 + geo['Ht'], 1:1 + geo['Wt']].cpu().numpy()
    assert (tile0[:9] == np.array(M.BG, dtype=np.uint8)).all()          # the clip of length 0 has no envelope


def _power(K, wave, lens):
    B, L = wave.shape
    power = torch.zeros(B, K.lt_frames(L), 129, device='cuda')
    nframes = torch.zeros(B, dtype=torch.int32, device='cuda')
    K.melcep_frames(wave, lens, nframes=nframes, power=power)
    return power, nframes


def test_sheet_writer_on_device_samples(K, tmp_path):
    from tests.test_sheet import read_png
    wave_h = _clips(6, 1000, [1000, 900, 64, 0, 512, 777], seed=9)
    wave, length = torch.from_numpy(wave_h).cuda(), torch.tensor([1000, 900, 64, 0, 512, 777]).cuda()
    w = sheet.SheetWriter(os.path.join(tmp_path, 's'), every=5, cols=4, Hw=10)
    assert w(4, wave, length, None) is None
    p = w(5, wave, length, None)
    assert os.path.basename(p) == 'sheet-5.png'
    assert np.array_equal(read_png(p), sheet.render(wave, length, cols=4, Hw=10).cpu().numpy())


def test_the_library_refuses(K):
    wave, power = torch.zeros(3, 384).cuda(), torch.zeros(3, 2, 129).cuda()
    nf, thr = torch.ones(3, dtype=torch.int32).cuda(), torch.from_numpy(sheet.thresholds()).cuda()
    cmap = torch.from_numpy(sheet.colormap()).cuda()
    img = torch.zeros(140, 13, 3, dtype=torch.uint8).cuda()
    K.sheet_render(wave, None, power, nf, thr, cmap, img, 3, 9, 1)
    for kw, what in ((dict(cols=2), 'sheet_geometry'), (dict(Hw=2), 'wave strip of 2'), (dict(gutter=17), 'gutter of 17')):
        a = dict(dict(cols=3, Hw=9, gutter=1), **kw)
        with pytest.raises(ValueError, match=what):
            K.sheet_render(wave, None, power, nf, thr, cmap, img, a['cols'], a['Hw'], a['gutter'])
    with pytest.raises(RuntimeError, match='img must be a CUDA'):
        K.sheet_render(wave, None, power, nf, thr, cmap, img.cpu(), 3, 9, 1)

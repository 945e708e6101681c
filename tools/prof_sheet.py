"""What does a sample sheet cost - a minibatch of ragged clips drawn as one image (ag_sheet_render, ``sheet.render``,
``sheet.SheetWriter``) - with the launch and with the stock form?

  * at (B 64, L 8192) and at (B 32, L 40000), random lengths between half a row and a whole one, 8 tiles across:
      ag_sheet_render   ``kernels.sheet_render`` alone, on the power ``kernels.melcep_frames`` left
      sheet.render      both launches into buffers that exist; nothing is read to the host
      the stock form    the same power launch, then torch ops: the lengths and frame counts read to the host, masked maxima,
                        ``log10``, clamp, ``bucketize``, an indexed colour table, the envelope rows by broadcast comparisons and
                        two slice assignments per clip
    device events around ``--launches`` back-to-back calls, the forms alternating, medians of ``--rounds`` rounds; microseconds,
    and for ag_sheet_render GB/s of samples and power read plus the image written.  The two forms' images are compared first:
    the share of pixels that differ is printed (a ``log10`` in fp32 and the exact threshold search part company where a cell
    sits on a level's edge).
  * ``SheetWriter`` end to end - both launches, the image copied to the host, the PNG deflated and written - on a host clock,
    beside one captured training pass at the C2 widths (tools/prof_eval.py's loop: 2 critic + 1 generator iteration, B 64).

    python tools/prof_sheet.py [--out profiles/sample_sheet.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, setup, timed          # noqa: E402

SHAPES = ((64, 8192), (32, 40000))
COLS, HW, GUTTER, RANGE_DB = 8, 64, 2, 80.0


def stock(wave, lens, power, nframes, cmap, edges_db, img, geo, colours):
    """the same sheet with stock torch, given the power: host reads of the lengths and frame counts, slices per clip"""
    bg, paper, ink = colours
    B, L = wave.shape
    n_h, nf_h = lens.cpu().tolist(), nframes.cpu().tolist()                      # the host reads
    t = torch.arange(L, device=wave.device)
    live = t[None, :] < lens[:, None]
    peak = (wave.abs() * live).amax(1)
    fr = torch.arange(power.size(1), device=wave.device)
    pmax = torch.where((fr[None, :] < nframes[:, None])[:, :, None], power, torch.zeros_like(power)).amax((1, 2))
    rel = 10.0 * torch.log10((power / pmax[:, None, None]).clamp(min=1e-30))
    level = (torch.bucketize(rel.clamp(-RANGE_DB, 0.0), edges_db, right=True) - 1).clamp(0, 255)
    Wt, Ht = geo['Wt'], geo['Ht']
    pad = Wt * 128 - L
    hi = torch.nn.functional.pad(torch.where(live, wave, torch.full_like(wave, -float('inf'))), (0, pad),
                                 value=-float('inf')).view(B, Wt, 128).amax(2)
    lo = torch.nn.functional.pad(torch.where(live, wave, torch.full_like(wave, float('inf'))), (0, pad),
                                 value=float('inf')).view(B, Wt, 128).amin(2)
    half = 0.5 * (HW - 1)
    r0 = torch.round((1.0 - hi / peak[:, None]) * half).clamp(0, HW - 1)
    r1 = torch.round((1.0 - lo / peak[:, None]) * half).clamp(0, HW - 1)
    rows = torch.arange(HW, device=wave.device, dtype=torch.float32)[None, :, None]
    inked = (rows >= r0[:, None, :]) & (rows <= r1[:, None, :])
    strip = torch.where(inked[..., None], ink, paper)                             # [B, Hw, Wt, 3]
    spec = cmap[level.permute(0, 2, 1).flip(1)]                                   # [B, 129, F, 3], bin 0 at the bottom
    img[...] = bg
    for b in range(B):
        y0 = GUTTER + (b // geo['cols']) * (Ht + GUTTER)
        x0 = GUTTER + (b % geo['cols']) * (Wt + GUTTER)
        ncol = (n_h[b] + 127) // 128
        img[y0:y0 + HW, x0:x0 + ncol] = strip[b, :, :ncol]
        img[y0 + HW:y0 + Ht, x0:x0 + nf_h[b]] = spec[b, :, :nf_h[b]]
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--writes', type=int, default=5)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'prof_sheet needs a GPU'
    from audiogan_amd import kernels as K
    from audiogan_amd import sheet
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say('sample sheets: us per call (device events around %d back-to-back calls), the forms alternating, medians of %d rounds'
        % (args.launches, args.rounds))
    thr = torch.from_numpy(sheet.thresholds(RANGE_DB)).to(dev)
    cmap = torch.from_numpy(sheet.colormap()).to(dev)
    edges_db = ((torch.arange(256, dtype=torch.float32) / 255.0 - 1.0) * RANGE_DB).to(dev)
    colours = tuple(torch.tensor(c, dtype=torch.uint8, device=dev) for c in (sheet.BG, sheet.PAPER, sheet.INK))
    for B, L in SHAPES:
        rs = np.random.RandomState(7)
        lens = torch.from_numpy(rs.randint(L // 2, L + 1, B).astype(np.int64)).to(dev)
        t = torch.arange(L, device=dev)
        wave = torch.randn(B, L, device=dev) * 0.2 * torch.sin(t[None, :] * (0.002 + 0.001 * torch.arange(B, device=dev)[:, None]))
        geo = sheet.sheet_geometry(B, L, COLS, HW, GUTTER)
        F = K.lt_frames(L)
        power = torch.empty(B, F, K.LTAS_BINS, device=dev)
        nframes = torch.empty(B, dtype=torch.int32, device=dev)
        img = torch.empty(geo['H'], geo['W'], 3, dtype=torch.uint8, device=dev)
        img_s = torch.empty_like(img)
        K.melcep_frames(wave, lens, nframes=nframes, power=power)

        def launch():
            K.sheet_render(wave, lens, power, nframes, thr, cmap, img, geo['cols'], HW, GUTTER)

        def render():
            sheet.render(wave, lens, cols=COLS, Hw=HW, gutter=GUTTER, out=img, power=power, nframes=nframes)

        def stock_form():
            K.melcep_frames(wave, lens, nframes=nframes, power=power)
            stock(wave, lens, power, nframes, cmap, edges_db, img_s, geo, colours)
        render()
        name = K.lib.ag_last_kernel().decode()
        stock_form()
        torch.cuda.synchronize()
        differ = float((img != img_s).any(2).float().mean())
        if differ > 0.02:
            say('WARNING: the forms differ in %.2f %% of the pixels' % (100 * differ))
        by = 4.0 * float(lens.sum()) + 4.0 * float(nframes.sum()) * K.LTAS_BINS + img.numel()
        tt = dict(l=[], r=[], s=[])
        for r in range(args.rounds):
            tt['l'].append(timed(launch, 5, args.launches) * 1e3)
            tt['r'].append(timed(render, 5, args.launches) * 1e3)
            tt['s'].append(timed(stock_form, 2, max(1, args.launches // 10)) * 1e3)
            say('B %d, L %d, round %d: ag_sheet_render %8.2f us   sheet.render %8.2f us   stock %10.2f us'
                % (B, L, r + 1, tt['l'][-1], tt['r'][-1], tt['s'][-1]))
        below = all(a < b for a, b in zip(tt['r'], tt['s']))
        say('B %d clips of up to %d samples (image %d x %d, %d workgroups; %.2f %% of the pixels differ between the forms): median '
            '%s %.2f us = %.1f GB/s of %.1f MB read + written, sheet.render (both launches, no host read) %.2f us;  the stock form '
            '(the same power launch, a host read of %d lengths and frame counts, %d slice assignments) %.2f us = %.1f x '
            'sheet.render;  sheet.render below the stock form in %s'
            % (B, L, geo['H'], geo['W'], geo['rows'] * geo['cols'] * ((geo['Wt'] + K.SHEET_TILE_COLUMNS - 1) // K.SHEET_TILE_COLUMNS),
               100 * differ, name, med(tt['l']), by / med(tt['l']) / 1e3, by / 1e6, med(tt['r']), B, 2 * B, med(tt['s']),
               med(tt['s']) / med(tt['r']), 'every round' if below else 'NOT every round'))
        if (B, L) == SHAPES[0]:
            keep = (wave, lens)
        del power, img, img_s

    # SheetWriter end to end beside a captured training pass
    wave, lens = keep
    folder = tempfile.mkdtemp(prefix='sheets')
    w = sheet.SheetWriter(folder, every=1, cols=COLS, Hw=HW, gutter=GUTTER)
    w(0, wave, lens, None)
    ev, lp = setup(64, 1, dev)
    for _ in range(3):
        lp.outer()          # two eager warm-up passes, the captures, one replayed pass
    torch.cuda.synchronize()
    t_w, t_d, t_p = [], [], []
    for r in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.writes):
            w(i + 1, wave, lens, None)
        t_w.append((time.perf_counter() - t0) * 1e3 / args.writes)
        t0 = time.perf_counter()
        for i in range(args.writes):
            host = w.sheet(wave, lens).cpu()          # the launches and the copy, without the file
        t_d.append((time.perf_counter() - t0) * 1e3 / args.writes)
        t_p.append(timed(lp.outer, 1, args.passes))
        say('round %d: SheetWriter (64 clips of up to 8192 samples -> one PNG on disk) %8.2f ms   of which launches and the copy '
            'to the host %8.2f ms   captured training pass %8.2f ms' % (r + 1, t_w[-1], t_d[-1], t_p[-1]))
    say('SheetWriter end to end (two launches, %.1f MB of image to the host, deflate, a file of %.0f KB): median %.2f ms on the host '
        'clock, %.2f ms of it the launches and the copy, the rest the host deflating and writing;  one captured training pass (C2 '
        'widths, B 64, 2 critic + 1 generator iteration) %.2f ms: a sheet costs %.2f passes'
        % (host.numel() / 1e6, os.path.getsize(w.written[-1]) / 1e3, med(t_w), med(t_d), med(t_p), med(t_w) / med(t_p)))
    K.check_persist_status(dev)
    for p in set(w.written):
        os.remove(p)
    os.rmdir(folder)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""What does the resampling launch of ingestion cost at sizes a user would run, beside what was there before it?

  * ``kernels.resample_poly`` (ag_resample_poly) at
        256 rows of 1 s at 16 kHz, int16 mono          (L / M = 1 / 2, 69 taps)
        8 rows of 60 s at 44.1 kHz, int16 stereo       (80 / 441, 187 taps)
        1 row of 600 s at 48 kHz, float mono           (1 / 6, 205 taps)
    device events around ``--launches`` back-to-back launches, every shape warmed up, the routes alternating, medians of
    ``--rounds`` rounds;
  * for the two integer-decimation sizes the stock device form ``torch.nn.functional.conv1d(x, bank, stride=M)`` on a mono
    float copy padded by half a filter either side (the copy and the padding are not timed); it cannot do the rational
    rates, the ragged rows or the int16 / stereo source.  The two results are compared;
  * for all three ``scipy.signal.resample_poly`` on the host, one thread, timed once with a host clock: a CPU BASELINE that
    stands for what the reference's librosa path does, not a kernel comparison (its filter is scipy's own);
  * achieved bytes/s, FMA/s and LDS reads/s from the shapes, and which of them bounds the kernel.  Peaks: 6.3 TB/s achievable
    HBM, 78.6 T fp32 FMA/s (157.3 TFLOPS), 18.75 T four-byte LDS reads/s (75 TB/s of ds_read_b32 with every CU streaming).

    python tools/prof_resample.py [--out profiles/ingest_resample.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, timed          # noqa: E402

PEAK_BYTES, PEAK_FMA, PEAK_LDS = 6.3e12, 78.6e12, 18.75e12
SIZES = (('256 rows of 1 s at 16 kHz, int16 mono', 16000, 256, 1.0, 1, np.int16),
         ('8 rows of 60 s at 44.1 kHz, int16 stereo', 44100, 8, 60.0, 2, np.int16),
         ('1 row of 600 s at 48 kHz, float mono', 48000, 1, 600.0, 1, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--scale', type=float, default=1.0, help='shrink the durations (a rehearsal)')
    ap.add_argument('--no-host', action='store_true', help='skip the scipy baseline')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'prof_resample needs a GPU: a CPU timing says nothing about the kernel'
    from audiogan_amd import audio
    from audiogan_amd import kernels as K
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    rs = np.random.RandomState(0)
    say('ag_resample_poly: ms per call, device events around %d back-to-back calls, medians of %d alternating rounds'
        % (args.launches, args.rounds))
    for title, sr, B, secs, C, dt in SIZES:
        n = int(sr * secs * args.scale)
        L, M, half, bank = audio.resample_bank(sr, device=dev)
        taps = bank.size(1)
        n_out = audio.out_count(n, L, M)
        x = rs.uniform(-1, 1, size=(B, n, C))
        x = (x * 30000).astype(np.int16) if dt is np.int16 else x.astype(np.float32)
        xs = torch.from_numpy(x).to(dev)
        src = xs if C > 1 else xs[:, :, 0]
        y = torch.empty(B, n_out, device=dev)
        run = lambda: K.resample_poly(src, None, bank, L, M, dst=y)          # noqa: E731
        run()
        assert K.lib.ag_last_kernel().decode() == 'resample_poly_kernel'
        stock = None
        if L == 1:
            mono = torch.nn.functional.pad(torch.from_numpy(audio.mono32(x.reshape(B * n, C)).reshape(B, 1, n)).to(dev),
                                           (half, half + M))
            w = bank.view(1, 1, taps)
            stock = lambda: torch.nn.functional.conv1d(mono, w, stride=M)          # noqa: E731
            ys = stock()[:, 0, :n_out]
            err = float((ys - y).abs().max())
            say('%s: conv1d and ag_resample_poly differ by at most %.2e (outputs of magnitude up to %.2f)'
                % (title, err, float(y.abs().max())))
        t = dict(k=[], s=[])
        for r in range(args.rounds):
            t['k'].append(timed(run, 3, args.launches))
            if stock is not None:
                t['s'].append(timed(stock, 3, args.launches))
        ms = med(t['k'])
        fma = float(B) * n_out * taps
        by = float(x.nbytes) + 4.0 * B * n_out + 4.0 * L * taps
        lds = fma * (1.25 if 256 % L == 0 else 2.0)          # four-byte LDS reads: 5 per 4 FMA when L divides 256, else 2 per FMA
        shares = dict(HBM=by / PEAK_BYTES, FMA=fma / PEAK_FMA, LDS=lds / PEAK_LDS)
        bound = max(shares, key=shares.get)
        say('%s (L / M = %d / %d, %d taps, %.1f M outputs): rounds %s' % (title, L, M, taps, B * n_out / 1e6,
                                                                          ' '.join('%.3f' % v for v in t['k'])))
        say('  ag_resample_poly %.3f ms = %.0f x real time;  %.2f TB/s of source + result,  %.2f T FMA/s,  %.2f T LDS reads/s;  '
            'least time by HBM %.3f ms, by FMA %.3f ms, by LDS reads %.3f ms: bound by %s, at %.0f %% of that bound'
            % (ms, B * secs * args.scale / (ms * 1e-3), by / (ms * 1e-3) / 1e12, fma / (ms * 1e-3) / 1e12,
               lds / (ms * 1e-3) / 1e12, shares['HBM'] * 1e3, shares['FMA'] * 1e3, shares['LDS'] * 1e3, bound,
               100.0 * shares[bound] * 1e3 / ms))
        if stock is not None:
            sm = med(t['s'])
            say('  conv1d(x, bank, stride=%d) on a padded mono float copy %.3f ms (rounds %s): ag_resample_poly / conv1d = %.3f%s'
                % (M, sm, ' '.join('%.3f' % v for v in t['s']), ms / sm,
                   '  -  the kernel is SLOWER than the stock form at this size' if ms > sm else ''))
        if not args.no_host:
            from scipy.signal import resample_poly
            xm = audio.mono32(x.reshape(B * n, C)).reshape(B, n)
            t0 = time.perf_counter()
            resample_poly(xm, L, M, axis=1)
            host = (time.perf_counter() - t0) * 1e3
            say('  CPU baseline, scipy.signal.resample_poly on one thread (its own filter; mono float input): %.1f ms = %.0f x '
                'real time;  ag_resample_poly is %.0f x that' % (host, B * secs * args.scale / (host * 1e-3), host / ms))
        del xs, src, y
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""What do the two activity launches of ingestion cost at sizes a user would run, beside the stock device form?

  * ``kernels.frame_power`` (ag_frame_power) and ``kernels.activity_segments`` (ag_activity_segments) at 8 kHz, 25 / 10 ms:
        256 rows of 1 s,   8 rows of 60 s,   1 row of 600 s
    device events around ``--launches`` back-to-back launches, every shape warmed up, the routes alternating, medians of
    ``--rounds`` rounds; achieved bytes/s against the rows read once (plus the powers written);
  * in the same run the stock device form ``x.unfold(1, win, hop).square().mean(-1)`` on rows zero-padded to whole frames
    (the padding is not timed).  It can take neither ragged rows with absolute starts nor promise chunk-independent bits;
    the run logic has no stock device form;
  * ``ingest.build_store(device='cuda')`` on a synthetic tree of ``--files`` one-second 16 kHz recordings with ``trim`` off
    and on: host seconds, medians of ``--rounds`` alternating rounds  ->  what trimming adds to an ingestion;
  * ``--fuzz``: the bound pass of tests/activity_model.py on the device, the largest |p - p64| / bound per shape.

    python tools/prof_activity.py [--out profiles/ingest_activity.txt] [--fuzz profiles/activity_fuzz.txt]
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

from tools.prof_eval import med, timed          # noqa: E402

SIZES = (('256 rows of 1 s', 256, 1.0), ('8 rows of 60 s', 8, 60.0), ('1 row of 600 s', 1, 600.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--out', default=None)
    ap.add_argument('--fuzz', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'prof_activity needs a GPU: a CPU timing says nothing about the kernels'
    from audiogan_amd import audio, ingest
    from audiogan_amd import kernels as K
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    q = audio.activity_params()
    win, hop = q['win'], q['hop']
    rs = np.random.RandomState(0)
    say('ag_frame_power / ag_activity_segments at 8 kHz, win %d hop %d (tile %d frames): ms per call, device events around %d '
        'back-to-back calls, medians of %d alternating rounds' % (win, hop, K.frame_power_tile(win, hop), args.launches, args.rounds))
    for title, B, secs in SIZES:
        n = int(8000 * secs)
        F = int(audio.frame_count(n, hop))
        x = rs.uniform(-1e-3, 1e-3, size=(B, n)).astype(np.float32)
        t = np.arange(n)
        x += (((t // 8000) % 2 == 0) & ((t % 8000) > 2400) & ((t % 8000) < 5600)) * np.where((t // 8) % 2 == 0, 0.5, -0.5).astype(np.float32)
        xs = torch.from_numpy(x).to(dev)
        padded = torch.nn.functional.pad(xs, (0, (F - 1) * hop + win - n))
        power = torch.empty(B, F, device=dev)
        nf = torch.full((B,), F, dtype=torch.int32, device=dev)
        ln = torch.full((B,), n, dtype=torch.int64, device=dev)
        seg = torch.full((B, 1024, 2), -1, dtype=torch.int64, device=dev)
        run_p = lambda: K.frame_power(xs, None, win, hop, dst=power)          # noqa: E731
        run_s = lambda: K.activity_segments(power, nf, ln, q['ratio'], q['floor'], q['min_gap'], q['min_run'], q['pad'], win, hop,  # noqa: E731
                                            K=1024, seg=seg)
        stock = lambda: padded.unfold(1, win, hop).square().mean(-1)          # noqa: E731
        run_p()
        assert K.lib.ag_last_kernel().decode() == 'frame_power_kernel'
        _, count, _ = run_s()
        ps = stock()
        err = float(((ps - power).abs() / power.clamp_min(1e-30)).max())
        tm = dict(p=[], s=[], u=[])
        for r in range(args.rounds):
            tm['p'].append(timed(run_p, 3, args.launches))
            tm['u'].append(timed(stock, 3, args.launches))
            tm['s'].append(timed(run_s, 3, args.launches))
        mp, mu, msg = med(tm['p']), med(tm['u']), med(tm['s'])
        by = 4.0 * B * n + 4.0 * B * F
        say('%s (%d frames a row, %d segments a row; unfold and ag_frame_power differ by at most %.1e relative):'
            % (title, F, int(count.max()), err))
        say('  ag_frame_power %.4f ms (rounds %s) = %.3f TB/s of rows read once + powers written'
            % (mp, ' '.join('%.4f' % v for v in tm['p']), by / (mp * 1e-3) / 1e12))
        say('  x.unfold(1, %d, %d).square().mean(-1) on padded rows %.4f ms (rounds %s): ag_frame_power / stock = %.3f%s'
            % (win, hop, mu, ' '.join('%.4f' % v for v in tm['u']), mp / mu,
               '  -  the kernel is SLOWER than the stock form at this size' if mp > mu else ''))
        say('  ag_activity_segments %.4f ms (rounds %s) = %.3f TB/s of powers read twice'
            % (msg, ' '.join('%.4f' % v for v in tm['s']), 8.0 * B * F / (msg * 1e-3) / 1e12))
        del xs, padded, power, seg

    # ---- what trimming adds to an ingestion --------------------------------------------------------------------------------
    from tests.ingest_model import pcm16, wav_bytes
    with tempfile.TemporaryDirectory() as root:
        for i in range(args.files):
            d = os.path.join(root, 'w%02d' % (i % 16))
            os.makedirs(d, exist_ok=True)
            y = rs.uniform(-30, 30, 16000)
            y[4800:11200] += 12000.0 * np.sin(2 * np.pi * 440.0 * np.arange(6400) / 16000.0)
            with open(os.path.join(d, 'f%04d.wav' % i), 'wb') as f:
                f.write(wav_bytes(pcm16(np.round(y)), 16000, 1, 16))
        entries = list(ingest.scan_tree(root))
        tm = dict(off=[], on=[])
        ingest.build_store(entries, device='cuda')
        ingest.build_store(entries, device='cuda', trim=True)
        for r in range(args.rounds):
            for key, kw in (('off', {}), ('on', dict(trim=True))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, rep = ingest.build_store(entries, device='cuda', **kw)
                tm[key].append(time.perf_counter() - t0)
        off, on = med(tm['off']), med(tm['on'])
        say('build_store(device=cuda) on %d files of 1 s at 16 kHz int16 (host clock, files in the page cache): trim off %.1f ms '
            '(rounds %s), trim on %.1f ms (rounds %s): trimming adds %.1f ms = %.0f %%; %.1f of %.1f s trimmed'
            % (args.files, off * 1e3, ' '.join('%.1f' % (v * 1e3) for v in tm['off']), on * 1e3,
               ' '.join('%.1f' % (v * 1e3) for v in tm['on']), (on - off) * 1e3, 100.0 * (on - off) / off, rep['seconds_trimmed'],
               rep['seconds_in']))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if args.fuzz:
        from tests import activity_model as M
        with open(args.fuzz, 'w') as f:
            f.write('ag_frame_power against float64 (the bound pass of tests/test_gpu_activity.py): the largest\n'
                    '|p - p64| / ((win + 3) 2^-24 p64 + 2^-100) over three launches of three ragged rows per shape, and at starts past 2^33\n')
            for win, hop in M.SHAPES:
                tile = K.frame_power_tile(win, hop)
                w = M.check_power_bound(K.frame_power, M.power_cases(win, hop, tile), on=lambda t: t.cuda())
                far = M.check_power_bound(K.frame_power, M.far_cases(win, hop), on=lambda t: t.cuda())
                f.write('win %4d hop %4d tile %3d: %.4f   far start: %.4f\n' % (win, hop, tile, w, far))


if __name__ == '__main__':
    main()

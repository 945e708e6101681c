"""What does the alignment launch cost beside the total alone, and how does that split into recording the decisions and
walking them back?

  * ``kernels.dtw_align`` against ``kernels.dtw_cost`` on the same pairs (what recording and walking back add), against the
    library's forward-only variant ``ag_dtw_align_forward`` (the same launch with the walk back compiled out: the difference
    is the walk), and against ``align.path64`` on the host for the same pairs;
  * at (64 pairs of 63 x 63 frames), (32 of 311 x 311) and (8 of 1024 x 1024), cepstra of noise clips from
    ``kernels.melcep_frames``; the totals of the three launches must have the same bits and the path must obey the path facts;
  * device events around ``--launches`` back-to-back launches, the routes alternating, medians of ``--rounds`` rounds.

    python tools/prof_dtwalign.py [--out profiles/ingest_align.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--host-pairs', type=int, default=2, help='pairs per shape that path64 is timed on')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from audiogan_amd import align
    from audiogan_amd import kernels as K
    from audiogan_amd.kernels import _p, _stream, check
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator().manual_seed(1)
    say('ag_dtw_align: us per launch, device events around %d back-to-back launches, rounds in the order they were taken'
        % args.launches)
    for B, L in ((64, 8192), (32, 40000), (8, 1023 * 128 + 256)):
        F = K.lt_frames(L)
        lens = torch.full((B,), L, dtype=torch.long, device=dev)
        nf = torch.empty(B, dtype=torch.int32, device=dev)
        ca = K.melcep_frames((torch.randn(B, L, generator=gen) * 0.3).to(dev), lens, nframes=nf)
        cb = K.melcep_frames((torch.randn(B, L, generator=gen) * 0.3).to(dev), lens)
        total, lo, hi = K.dtw_align(ca, nf, cb, nf)
        fwd, cost = torch.empty_like(total), torch.empty_like(total)
        ws = torch.empty(B * K.dtw_align_ws(F, F) // 4, dtype=torch.int32, device=dev)

        def forward_only():
            check(K.lib.ag_dtw_align_forward(_p(ca), _p(nf), _p(cb), _p(nf), _p(fwd), _p(lo), _p(hi), _p(ws), ws.numel() * 4, B,
                                             F, F, _stream()), 'ag_dtw_align_forward')

        forward_only()
        K.dtw_cost(ca, nf, cb, nf, out=cost)
        bits = lambda t: t.view(torch.int32)          # noqa: E731
        assert torch.equal(bits(total), bits(cost)) and torch.equal(bits(fwd), bits(cost)), 'the totals differ'
        total, lo, hi = K.dtw_align(ca, nf, cb, nf, workspace=ws)
        l, h = lo.cpu().numpy().astype(np.int64), hi.cpu().numpy().astype(np.int64)
        assert (l[:, 0] == 0).all() and (h[:, -1] == F - 1).all() and (l <= h).all()
        assert np.isin(l[:, 1:] - h[:, :-1], (0, 1)).all()
        say('%d pairs of %d x %d frames (workspace %.0f KB a pair): the three launches give the same totals'
            % (B, F, F, K.dtw_align_ws(F, F) / 1024.0))
        t = dict(align=[], fwd=[], cost=[])
        for r in range(args.rounds):
            t['align'].append(timed(lambda: K.dtw_align(ca, nf, cb, nf, total=total, lo=lo, hi=hi, workspace=ws), 5,
                                    args.launches) * 1e3)
            t['fwd'].append(timed(forward_only, 5, args.launches) * 1e3)
            t['cost'].append(timed(lambda: K.dtw_cost(ca, nf, cb, nf, out=cost), 5, args.launches) * 1e3)
            say('round %d  dtw_align %10.2f   forward only %10.2f   dtw_cost %10.2f' % (r + 1, t['align'][-1], t['fwd'][-1],
                                                                                         t['cost'][-1]))
        a, f, c = med(t['align']), med(t['fwd']), med(t['cost'])
        cah, cbh = ca.cpu().numpy(), cb.cpu().numpy()
        host = []
        for b in range(min(B, max(1, args.host_pairs))):
            t0 = time.perf_counter()
            want = align.path64(cah[b], F, cbh[b], F)
            host.append((time.perf_counter() - t0) * 1e6)
            same = np.array_equal(want[1], l[b]) and np.array_equal(want[2], h[b])
            say('  path64 on the host, pair %d: %.0f us; its path is %s the launch\'s' % (b, host[-1], 'the same as' if same
                                                                                          else 'NOT'))
        say('median: dtw_align %.2f us (%.2f us a pair);  forward only %.2f us;  dtw_cost %.2f us;  dtw_align / dtw_cost = %.3f;  '
            'recording the decisions (forward only - dtw_cost) %.2f us = %.1f %% of dtw_align;  the walk back (dtw_align - '
            'forward only) %.2f us = %.1f %%;  path64 on the host %.0f us a pair = %.0f x the launch\'s time a pair'
            % (a, a / B, f, c, a / c, f - c, 100.0 * (f - c) / a, a - f, 100.0 * (a - f) / a, med(host), med(host) / (a / B)))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

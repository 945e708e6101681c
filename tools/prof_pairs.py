"""What does the all-pairs DTW launch cost beside what the library offered before it, and what do the crossed keys and the extra
draws add to an evaluation pass?

  * ``kernels.dtw_pairs`` as a cross product at (64 x 64 sequences of 63 frames: the wave form) and (32 x 32 of 311 frames:
    the workgroup form) against the paired route: a gather of both banks to P rows (timed on its own) plus one
    ``kernels.dtw_cost`` launch of P pairs; the results must have the same bits.  Device events around ``--launches``
    back-to-back launches, the routes alternating, medians of ``--rounds`` rounds;
  * one ``evaluate.Evaluator.run()`` at the C2 widths (the setup of tools/prof_eval.py, full-length fakes) with ``aligned``
    alone, with ``crossed``, and with ``crossed`` and ``draws=2``, alternating.

    python tools/prof_pairs.py [--out profiles/eval_pairs.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, setup, timed          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from audiogan_amd import evaluate
    from audiogan_amd import kernels as K
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator().manual_seed(1)
    say('all-pairs DTW: us per call, device events around %d back-to-back calls, rounds in the order they were taken'
        % args.launches)
    for N, L in ((64, 8192), (32, 40000)):
        F = K.lt_frames(L)
        lens = torch.full((N,), L, dtype=torch.long, device=dev)
        nf = torch.empty(N, dtype=torch.int32, device=dev)
        ca = K.melcep_frames((torch.randn(N, L, generator=gen) * 0.3).to(dev), lens, nframes=nf)
        cb = K.melcep_frames((torch.randn(N, L, generator=gen) * 0.3).to(dev), lens)
        I = torch.arange(N, device=dev).repeat_interleave(N)
        J = torch.arange(N, device=dev).repeat(N)
        P = N * N
        out = torch.empty(N, N, device=dev)
        paired = torch.empty(P, device=dev)
        held = {}

        def gather():
            held['g'] = (ca[I], nf[I], cb[J], nf[J])

        gather()
        K.dtw_pairs(ca, nf, cb, nf, out=out)
        form = K.lib.ag_last_kernel().decode()
        K.dtw_cost(*held['g'], out=paired)
        assert torch.equal(out.view(-1).view(torch.int32), paired.view(torch.int32)), 'dtw_pairs and dtw_cost differ'
        say('%d x %d sequences of %d frames (%d pairs, %s; gathered banks %.1f MB): the same bits by both routes'
            % (N, N, F, P, form, 2.0 * P * F * 64 / 1e6))
        t = dict(pairs=[], gather=[], cost=[])
        for r in range(args.rounds):
            t['pairs'].append(timed(lambda: K.dtw_pairs(ca, nf, cb, nf, out=out), 5, args.launches) * 1e3)
            t['gather'].append(timed(gather, 5, args.launches) * 1e3)
            t['cost'].append(timed(lambda: K.dtw_cost(*held['g'], out=paired), 5, args.launches) * 1e3)
            say('round %d  dtw_pairs %10.2f   gather to P rows %10.2f   dtw_cost of P pairs %10.2f   gather + dtw_cost %10.2f   '
                'dtw_pairs %s' % (r + 1, t['pairs'][-1], t['gather'][-1], t['cost'][-1], t['gather'][-1] + t['cost'][-1],
                                  'not slower' if t['pairs'][-1] <= t['gather'][-1] + t['cost'][-1] else 'SLOWER'))
        say('median: dtw_pairs %.2f us (%.1f ns per pair);  gather %.2f us;  dtw_cost %.2f us;  gather + dtw_cost %.2f us;  '
            'dtw_pairs / (gather + dtw_cost) = %.3f,  dtw_pairs / dtw_cost alone = %.3f'
            % (med(t['pairs']), med(t['pairs']) * 1e3 / P, med(t['gather']), med(t['cost']), med(t['gather']) + med(t['cost']),
               med(t['pairs']) / (med(t['gather']) + med(t['cost'])), med(t['pairs']) / med(t['cost'])))

    ev, lp = setup(args.batch, args.batches, dev)
    heldout = [(0, 0, mb['real'].cpu().numpy(), mb['real_len'].cpu().numpy(), None, mb['cs'].cpu().numpy(),
                mb['cl'].cpu().numpy()) for mb in ev.set]
    evs = [evaluate.Evaluator(ev.g, ev.d, ev.e_g, ev.e_d, heldout, ev.B, ev.maxlen, dev, batches=args.batches, seed=0,
                              aligned=True, **kw) for kw in ({}, dict(crossed=True), dict(crossed=True, draws=2))]
    for e in evs:          # full-length fakes, the long end: no stop draw falls below its probability
        for mb in e.set:
            mb['u'].fill_(1.0)
            for _, u in mb.get('more', ()):
                u.fill_(1.0)
    res = evs[2].run()
    say('Evaluator.run() at the C2 widths, %d clips per minibatch, %d held-out minibatches, full-length fakes (%.1f frames of '
        '%d); ms per pass, device events around %d passes ending in a synchronise;  untrained: mcd_db %.2f, nn_db %.2f, '
        'cover_db %.2f, word_hit %.3f (chance %.3f), div_db %.2f, real_div_db %s'
        % (args.batch, args.batches, res['frames/mean'], ev.nframes, args.passes, res['mcd_db'], res['nn_db'], res['cover_db'],
           res['word_hit'], res['word_hit/chance'], res['div_db'],
           'None' if res['real_div_db'] is None else '%.2f' % res['real_div_db']))
    t = [[], [], []]
    for r in range(args.rounds):
        for k, e in enumerate(evs):
            t[k].append(timed(e.run, 1, args.passes))
        say('round %d  aligned %9.2f   aligned + crossed %9.2f   aligned + crossed + draws=2 %9.2f' % (r + 1, t[0][-1], t[1][-1],
                                                                                                    t[2][-1]))
    say('median: aligned %.2f ms;  + crossed %.2f ms: +%.2f ms per pass (+%.3f per held-out minibatch);  + crossed + draws=2 '
        '%.2f ms: +%.2f ms per pass (+%.3f per held-out minibatch)'
        % (med(t[0]), med(t[1]), med(t[1]) - med(t[0]), (med(t[1]) - med(t[0])) / args.batches, med(t[2]),
           med(t[2]) - med(t[0]), (med(t[2]) - med(t[0])) / args.batches))
    K.check_persist_status(dev)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

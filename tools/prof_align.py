"""What do the two kernels of the aligned distance cost, how close are they to float64, and what does the option add to a pass?

  * ``kernels.melcep_frames`` at (B 64, L 8192) and (B 32, L 40000) against ``kernels.ltas_power`` on the same clips (the
    direct DFT on the vector unit, which does a subset of the work: no per-frame output, no mel sums, no logarithm) and
    against the stock form (``torch.stft``, |X|^2, two ``matmul``s and a ``log``), alternating in the same run; device events
    around ``--launches`` back-to-back launches, medians of ``--rounds`` rounds;
  * ``kernels.dtw_cost`` at 63 and 311 frames a side (the frame counts of those two clip lengths), the same way;
  * the measured error / floor ratios of the cases of tests/align_model.py (what the tests bound);
  * one ``evaluate.Evaluator.run()`` at the C2 widths (the setup of tools/prof_eval.py) with ``aligned`` off and on, alternating.

    python tools/prof_align.py [--out profiles/eval_aligned.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.prof_eval import med, setup, timed          # noqa: E402


def stock_melcep(x, win, mel, dct):
    s = torch.stft(x, 256, hop_length=128, win_length=256, window=win, center=False, return_complex=True)
    p = (s.real ** 2 + s.imag ** 2).transpose(1, 2)
    return torch.log(torch.matmul(p, mel.t()) + 1e-10) @ dct.t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from audiogan_amd import evaluate
    from audiogan_amd import kernels as K
    from tests import align_model
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator().manual_seed(1)
    win = torch.hann_window(256, periodic=True, device=dev)
    mel, dct = K.mel_table(device=dev), K.dct_table(device=dev)
    say('aligned distance: us per launch, device events around %d back-to-back launches, rounds in the order they were taken'
        % args.launches)
    for B, L in ((64, 8192), (32, 40000)):
        x = (torch.randn(B, L, generator=gen) * 0.3).to(dev)
        lens = torch.full((B,), L, dtype=torch.long, device=dev)
        F = K.lt_frames(L)
        out = torch.empty(B, K.LTAS_BINS, device=dev)
        cep = torch.empty(B, F, K.CEP_WIDTH, device=dev)
        nf = torch.empty(B, dtype=torch.int32, device=dev)
        K.melcep_frames(x, lens, cep=cep, nframes=nf)
        ref = stock_melcep(x, win, mel, dct)
        err = float((cep[:, :, :K.MEL_NCEP] - ref).abs().max() / ref.abs().max())
        say('B %d, L %d (%d frames per clip); melcep_frames against the stock form: largest difference %.1e of the largest |c|'
            % (B, L, F, err))
        t = dict(mc=[], lt=[], st=[], dtw=[])
        cb = cep.flip(0).contiguous()
        dtw = torch.empty(B, device=dev)
        for r in range(args.rounds):
            t['mc'].append(timed(lambda: K.melcep_frames(x, lens, cep=cep, nframes=nf), 10, args.launches) * 1e3)
            t['lt'].append(timed(lambda: K.ltas_power(x, lens, out=out), 10, args.launches) * 1e3)
            t['st'].append(timed(lambda: stock_melcep(x, win, mel, dct), 10, args.launches) * 1e3)
            t['dtw'].append(timed(lambda: K.dtw_cost(cep, nf, cb, nf, out=dtw), 10, args.launches) * 1e3)
            say('round %d  melcep_frames %9.2f   ltas_power %9.2f   torch.stft + |X|^2 + 2 matmul + log %9.2f   dtw_cost (%d x %d '
                'frames) %9.2f' % (r + 1, t['mc'][-1], t['lt'][-1], t['st'][-1], F, F, t['dtw'][-1]))
        flop = 2.0 * 2 * 256 * 129 * F * B
        say('median: melcep_frames %.2f us (%.2f TFLOP/s counted as the direct DFT, 2 * 2 * 256 * 129 per frame; the folded form '
            'issues half);  ltas_power %.2f us;  melcep_frames / ltas_power = %.2f;  stock form %.2f us;  library / stock = %.2f;  '
            'dtw_cost %.2f us (%.1f ns per anti-diagonal)'
            % (med(t['mc']), flop / med(t['mc']) / 1e6, med(t['lt']), med(t['mc']) / med(t['lt']), med(t['st']),
               med(t['mc']) / med(t['st']), med(t['dtw']), med(t['dtw']) * 1e3 / (2 * F - 1)))
    say('error / floor ratios of the test cases (tests/align_model.py: bound %g; power: fraction of the frame\'s largest bin, '
        'bound %g):' % (align_model.CEP_MARGIN, align_model.LTAS_BOUND))
    for kind, size in align_model.MELCEP_CASES:
        r = align_model.run_melcep(K.melcep_frames, K.ltas_power, kind, size, on=lambda t_: t_.to(dev))
        say('  melcep_frames %-5s %-5s  teacher-forced %.2f   end to end %s   power %.2e' %
            (kind, size, r['forced'], '%.2f' % r['e2e'] if 'e2e' in r else '  - ', r['power']))
    say('  dtw_cost real pass: largest |D32 - D64| / bound %.3f'
        % align_model.check_dtw_real(K.dtw_cost, on=lambda t_: t_.to(dev)))

    ev, lp = setup(args.batch, args.batches, dev)
    heldout = [(0, 0, mb['real'].cpu().numpy(), mb['real_len'].cpu().numpy(), None, mb['cs'].cpu().numpy(),
                mb['cl'].cpu().numpy()) for mb in ev.set]
    ev2 = evaluate.Evaluator(ev.g, ev.d, ev.e_g, ev.e_d, heldout, ev.B, ev.maxlen, dev, batches=args.batches, seed=0,
                             aligned=True)
    for mb in ev2.set:          # full-length fakes, the long end for the new kernels: no stop draw falls below its probability
        mb['u'].fill_(1.0)
    for mb in ev.set:
        mb['u'].fill_(1.0)
    res = ev2.run()
    say('Evaluator.run() at the C2 widths, %d clips per minibatch, %d held-out minibatches, full-length fakes (%.1f frames of '
        '%d); ms per pass, device events around %d passes ending in a synchronise;  mcd_db %.2f, ltas_db %.2f (untrained)'
        % (args.batch, args.batches, res['frames/mean'], ev.nframes, args.passes, res['mcd_db'], res['ltas_db']))
    t_off, t_on = [], []
    for r in range(args.rounds):
        t_off.append(timed(ev.run, 1, args.passes))
        t_on.append(timed(ev2.run, 1, args.passes))
        say('round %d  aligned off %9.2f   aligned on %9.2f' % (r + 1, t_off[-1], t_on[-1]))
    say('median: aligned off %.2f ms, on %.2f ms: +%.2f ms per pass (+%.3f per held-out minibatch)'
        % (med(t_off), med(t_on), med(t_on) - med(t_off), (med(t_on) - med(t_off)) / args.batches))
    K.check_persist_status(dev)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

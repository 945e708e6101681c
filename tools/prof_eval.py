"""What does a held-out evaluation pass cost, and what do its two kernels cost alone?

  * one ``evaluate.Evaluator.run()`` at the C2 widths (state 1024, frame 256, 8192-sample ragged clips from the loader
    interface), ``--batch`` clips per minibatch and ``--batches`` held-out minibatches, beside one training pass of the same
    networks (``TrainLoop(graphed=True, fixed_critic_iter=2)``: two critic iterations and one generator iteration, what
    bench.py --workload full times), and the same evaluation with every stop uniform set to 1 (full-length fakes: an
    untrained stop head ends its clips after a frame or two) - the three alternate ``--rounds`` times, each timed with device
    events around whole passes that end in a synchronise;
  * ``kernels.ltas_power`` and ``kernels.score_accum`` alone at (B 64, L 8192) and (B 32, L 40000), device events around
    ``--launches`` back-to-back launches, alternating with the same spectrum through ``torch.stft`` (window, |X|^2, mean over
    the frames; fixed-length clips, which is all it can do in one call) for context.

    python tools/prof_eval.py [--out profiles/eval_pass.txt]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, launches):
    """-> milliseconds per call: device events around ``launches`` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def med(v):
    return sorted(v)[len(v) // 2]


def setup(B, batches, dev):
    import audiogan_amd as A
    from audiogan_amd import dataset as D
    from audiogan_amd import evaluate, loop, optim
    torch.manual_seed(0)
    frame, maxlen = 256, 8192
    g = A.Generator(frame_size=frame, embed_size=100, noise_size=100, state_size=1024, num_layers=1).to(dev)
    d = A.Discriminator(state_size=1024, embed_size=100, num_layers=1).to(dev)
    e_g, e_d = (A.Embedder(output_size=100, char_embed_size=50, num_layers=1, num_chars=256).to(dev) for _ in range(2))
    opt_g = optim.make_optimizer(list(g.parameters()) + list(e_g.parameters()), 'rmsprop', 1e-4)
    opt_d = optim.make_optimizer(list(d.parameters()) + list(e_d.parameters()), 'rmsprop', 1e-4)
    words = ['word%02d' % i for i in range(40)]
    ds = D.SyntheticWordDataset(words, n_per_word=4, min_len=maxlen // 3, max_len=maxlen, kind='noise', seed=3)
    args = types.SimpleNamespace(conditional=True, dataset=ds, minwordlen=1, subset=None, amplitudes=0)
    np.random.seed(5)
    h5, ml, gen_train, gen_valid, keys_train, _ = D.dataloader(B, args, maxlen=maxlen, frame_size=frame)
    ev = evaluate.Evaluator(g, d, e_g, e_d, gen_valid, B, ml, dev, batches=batches, seed=0)      # (before the first training next())
    pick = loop.words_picker(D, B, ml, h5, keys_train, args, frame_size=frame)
    lp = loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, B, ml, dev, fixed_critic_iter=2, gencatchup=1,
                        stop='never', checkpoint_every=0, check=False, graphed=True)
    return ev, lp


def stft_ltas(x, win):
    s = torch.stft(x, 256, hop_length=128, win_length=256, window=win, center=False, return_complex=True)
    return (s.real ** 2 + s.imag ** 2).mean(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from audiogan_amd import kernels as K
    dev = torch.device('cuda')
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    ev, lp = setup(args.batch, args.batches, dev)
    for _ in range(3):
        lp.outer()          # two eager warm-up passes, the captures, one replayed pass
    res = ev.run()
    say('held-out evaluation at the C2 widths, %d clips per minibatch, %d held-out minibatches (%d clips); ms per pass, device '
        'events around %d passes ending in a synchronise; rounds in the order they were taken' %
        (args.batch, args.batches, ev.clips, args.passes))
    say('(untrained networks: mean generated length %.1f frames of %d - the short end; the second column sets every stop uniform '
        'to 1, so every fake runs all its frames - the long end)' % (res['frames/mean'], ev.nframes))
    t_ev, t_long, t_tr = [], [], []
    short = [mb['u'].clone() for mb in ev.set]

    def with_u(us):
        for mb, u in zip(ev.set, us):
            mb['u'].copy_(u)

    for r in range(args.rounds):
        with_u(short)
        t_ev.append(timed(ev.run, 1, args.passes))
        with_u([torch.ones_like(u) for u in short])          # no stop draw ever falls below its probability: full-length fakes
        t_long.append(timed(ev.run, 1, args.passes))
        t_tr.append(timed(lp.outer, 1, args.passes))
        say('round %d  Evaluator.run() %9.2f   with full-length fakes %9.2f   training pass (captured, 2 critic + 1 generator '
            'iteration) %9.2f' % (r + 1, t_ev[-1], t_long[-1], t_tr[-1]))
    say('median: Evaluator.run() %.2f ms (%.2f ms per held-out minibatch), with full-length fakes %.2f ms (%.2f);  training pass '
        '%.2f ms;  evaluation / training pass = %.2f, full-length %.2f  (spread of the evaluation rounds %.2f .. %.2f ms, '
        'full-length %.2f .. %.2f ms)'
        % (med(t_ev), med(t_ev) / args.batches, med(t_long), med(t_long) / args.batches, med(t_tr), med(t_ev) / med(t_tr),
           med(t_long) / med(t_tr), min(t_ev), max(t_ev), min(t_long), max(t_long)))
    K.check_persist_status(dev)
    del ev, lp
    gen = torch.Generator().manual_seed(1)
    win = torch.hann_window(256, periodic=True, device=dev)
    for B, L in ((64, 8192), (32, 40000)):
        x = (torch.randn(B, L, generator=gen) * 0.3).to(dev)
        lens = torch.full((B,), L, dtype=torch.long, device=dev)
        out = torch.empty(B, K.LTAS_BINS, device=dev)
        ref = stft_ltas(x, win)
        err = float((K.ltas_power(x, lens, out=out) - ref).abs().max() / ref.abs().max())
        cls = torch.randn(B, L // 64, generator=gen).to(dev)
        nf = torch.full((B,), L // 64, dtype=torch.long, device=dev)
        acc = torch.zeros(K.SCORE_WORDS, dtype=torch.float64, device=dev)
        frames = (L - 256) // 128 + 1
        say('B %d, L %d (%d frames per clip; logits [%d, %d]); us per launch, device events around %d back-to-back launches; '
            'ltas_power against torch.stft: largest difference %.1e of the largest bin'
            % (B, L, frames, B, L // 64, args.launches, err))
        t = dict(ltas=[], stft=[], score=[])
        for r in range(args.rounds):
            t['ltas'].append(timed(lambda: K.ltas_power(x, lens, out=out), 10, args.launches) * 1e3)
            t['stft'].append(timed(lambda: stft_ltas(x, win), 10, args.launches) * 1e3)
            t['score'].append(timed(lambda: K.score_accum(cls, nf, 0.9, True, acc), 10, args.launches) * 1e3)
            say('round %d  ltas_power %9.2f   torch.stft + |X|^2 + mean %9.2f   score_accum %9.2f'
                % (r + 1, t['ltas'][-1], t['stft'][-1], t['score'][-1]))
        flop = 2.0 * 2 * 256 * 129 * frames * B
        say('median: ltas_power %.2f us (%.2f TFLOP/s of the direct DFT: 2 * 2 * 256 * 129 per frame);  torch.stft form %.2f us;  '
            'library / stock = %.2f;  score_accum %.2f us' % (med(t['ltas']), flop / med(t['ltas']) / 1e6, med(t['stft']),
                                                             med(t['ltas']) / med(t['stft']), med(t['score'])))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

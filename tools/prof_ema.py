"""What does one EMA update of the generator's weights cost, against the stock one-liner?

The parameter list of the default ``Generator(embed_size=100)`` plus ``Embedder(100)`` (what ``opt_g`` holds) on the GPU.
After ``--warmup`` launches, ``--launches`` back-to-back ``optim.EMA.update()`` launches (one ag_ema_update each) are timed
with HIP events; in the same process, the same way, ``torch._foreach_lerp_(shadows, params, 1 - decay)`` over the same
tensors.  The two alternate ``--rounds`` times.  Issued from Python both figures contain the host's enqueue pace, so each
is also timed as ONE hipGraph of ``--launches`` launches (what a captured TrainLoop pays: the device time alone).

    python tools/prof_ema.py [--out profiles/ema_update.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, launches):
    """-> microseconds per launch: HIP events around ``launches`` back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def graphed(fn, launches):
    """``launches`` calls captured into one graph -> a callable that replays it"""
    from audiogan_amd import common, kernels as K
    K.reserve_table_arena()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    common.new_capture()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    return gr.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import audiogan_amd as A
    from audiogan_amd import optim
    dev = torch.device('cuda')
    torch.manual_seed(0)
    g, e_g = A.Generator(embed_size=100).to(dev), A.Embedder(100).to(dev)
    params = list(g.parameters()) + list(e_g.parameters())
    opt = optim.make_optimizer(params, 'rmsprop', 1e-4)
    ema = optim.EMA(opt, decay=args.decay, warmup=True)
    n = sum(p.numel() for p in params)
    # the stock alternative keeps shadows of its own (same sizes, separately allocated as a user's clones would be)
    sh = [p.detach().clone() for p in params]
    ps = [p.detach() for p in params]
    w = 1.0 - args.decay
    ours = ema.update
    stock = lambda: torch._foreach_lerp_(sh, ps, w)      # noqa: E731
    lines = ['EMA update of %d tensors, %d elements (%.1f MB moved per update: 12 bytes per element); us per launch, HIP events '
             'around %d back-to-back launches after %d warm-up launches; rounds in the order they were taken'
             % (len(params), n, 12.0 * n / 1e6, args.launches, args.warmup)]
    lines.append('(both tensor lists together stay inside the 256 MiB Infinity Cache from one launch to the next: the rates below '
                 'are not HBM rates)')
    res = dict(ours=[], stock=[], ours_graph=[], stock_graph=[])
    for r in range(args.rounds):
        res['ours'].append(timed(ours, args.warmup, args.launches))
        res['stock'].append(timed(stock, args.warmup, args.launches))
        lines.append('round %d  issued from Python:  ema.update() %8.2f   torch._foreach_lerp_ %8.2f'
                     % (r + 1, res['ours'][-1], res['stock'][-1]))
        print(lines[-1], flush=True)
    go, gs = graphed(ours, args.launches), graphed(stock, args.launches)
    for r in range(args.rounds):
        res['ours_graph'].append(timed(go, 2, 3) / args.launches)
        res['stock_graph'].append(timed(gs, 2, 3) / args.launches)
        lines.append('round %d  one graph of %d:      ema.update() %8.2f   torch._foreach_lerp_ %8.2f'
                     % (r + 1, args.launches, res['ours_graph'][-1], res['stock_graph'][-1]))
        print(lines[-1], flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    for tag, a, b in (('issued from Python', 'ours', 'stock'), ('captured', 'ours_graph', 'stock_graph')):
        lines.append('%-18s median: ema.update() %.2f us = %.2f TB/s (12 N / t);  torch._foreach_lerp_ %.2f us = %.2f TB/s;  '
                     'library / stock = %.2f  (spread of the library rounds %.2f .. %.2f us)'
                     % (tag, med[a], 12.0 * n / med[a] / 1e6, med[b], 12.0 * n / med[b] / 1e6, med[a] / med[b],
                        min(res[a]), max(res[a])))
    lines.append('condition (the library launch is not slower than the stock one, issued from Python): %s;  captured: %s'
                 % ('met' if med['ours'] <= med['stock'] else 'NOT met',
                    'met' if med['ours_graph'] <= med['stock_graph'] else 'NOT met'))
    print('\n'.join(lines[-3:]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

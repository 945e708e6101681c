"""What do the per-iteration summaries cost a captured loop?

The captured ``loop.TrainLoop`` of ``bench.py --workload full`` (C2 widths, 2 critic iterations + 1 generator iteration per pass,
ragged loader clips) with ``summary`` off and on, alternating in ONE process (off, on, off, on: clocks and allocator state drift
together), wall milliseconds per pass over ``--passes`` passes per block, ``--blocks`` blocks per run.  With ``summary`` on the
loop also drains the ring (every ``capacity // 2`` iterations and at the end): the host read is part of the figure.

    python tools/prof_summary.py --batch 64 --passes 20 --blocks 3 [--out profiles/loop_summaries.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_run(args, on, dev):
    import audiogan_amd as A
    import bench
    from audiogan_amd import kernels as K, loop, optim
    from audiogan_amd.summary import Summary
    mods, (D, h5, maxlen, gen_train, keys_train, a) = bench._full_setup(A, optim, dev, args.batch, 'rmsprop')
    g, d, e_g, e_d, opt_g, opt_d = mods
    pick = loop.words_picker(D, args.batch, maxlen, h5, keys_train, a, frame_size=bench.FRAME)
    rows = []
    kw = dict(summary=Summary(dev, capacity=256, on_row=rows.append)) if on else {}
    lp = loop.TrainLoop(g, d, e_g, e_d, opt_g, opt_d, gen_train, pick, args.batch, maxlen, dev, fixed_critic_iter=2,
                        gencatchup=1, stop='never', checkpoint_every=0, check=False, graphed=True, **kw)
    lp.outer()                        # two eager warm-up passes, the three captures, one replayed pass
    lp.outer()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        for _ in range(args.passes):
            lp.outer()
        if on:
            lp.drain_summary()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / args.passes * 1e3)
    assert K.lstm_persist_status(dev) == 0
    if on:
        assert len(rows) == 3 * (4 + args.blocks * args.passes), len(rows)
    return blocks, (rows[-3:] if on else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--runs', type=int, default=2, help='runs of each setting, alternating off / on')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = ['captured TrainLoop, C2 widths, batch %d: wall ms per pass (2 critic + 1 generator iteration), %d passes per block; '
             'runs in the order they were taken' % (args.batch, args.passes)]
    res = {False: [], True: []}
    last = None
    for i in range(2 * args.runs):
        on = bool(i % 2)
        blocks, rows = one_run(args, on, dev)
        res[on].append(blocks)
        last = rows or last
        lines.append('run %d  summary %-3s  %s   min %.3f' % (i + 1, 'on' if on else 'off', '  '.join('%.3f' % b for b in blocks),
                                                           min(blocks)))
        print(lines[-1], flush=True)
    off = [min(b) for b in res[False]]
    on_ = [min(b) for b in res[True]]
    m_off, m_on = sum(off) / len(off), sum(on_) / len(on_)
    all_off = [x for b in res[False] for x in b]
    lines.append('off: mean of the runs\' best blocks %.3f ms, spread of all off blocks %.3f ms (%.3f .. %.3f)'
                 % (m_off, max(all_off) - min(all_off), min(all_off), max(all_off)))
    lines.append('on : mean of the runs\' best blocks %.3f ms;  on - off = %+.3f ms = %+.2f %% of a pass'
                 % (m_on, m_on - m_off, 100.0 * (m_on - m_off) / m_off))
    lines.append('accept: on - off <= spread of the off blocks + 1 %% of a pass = %.3f ms: %s'
                 % (max(all_off) - min(all_off) + 0.01 * m_off,
                    'yes' if m_on - m_off <= max(all_off) - min(all_off) + 0.01 * m_off else 'NO'))
    if last:
        lines.append('last rows: ' + '; '.join(str(r) for r in last))
    print('\n'.join(lines[-4:]))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Are the kernel names of ``bench.py --full``'s kernel_table the names rocprofv3 gives the same kernels?

    python tools/kernel_names_vs_trace.py LINE.json STATS.csv [LABEL]

LINE.json: the JSON result line of ``python bench.py --full`` (the last line of the file that parses is taken);
STATS.csv: ``*_kernel_stats.csv`` of ``rocprofv3 --kernel-trace --stats -- python bench.py --steps 2 --warmup 1 --no-graph
--no-roofline`` with the same --dtype.  Every kernel_table row whose name starts with ``gemm`` or ``conv_`` must be in the
trace's Name column once ``void ``, the parameter list and spaces are removed from the latter.  The trace command runs 3
steps (1 warm-up + 2), so a name that is right also has 3 x the row's launches per step as its Calls there: a name that
exists but is given to calls that ran another kernel shows up as a count that does not match.  Prints one row per name
and exits 1 when a name is missing or a count differs."""
import csv
import json
import sys

TRACE_STEPS = 3


def trace_names(path):
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            n = row['Name']
            if n.startswith('void '):
                n = n[5:]
            if n.endswith(')'):                      # the parameter list: from the '(' that matches the last ')'
                depth = 0
                for i in range(len(n) - 1, -1, -1):
                    depth += (n[i] == ')') - (n[i] == '(')
                    if depth == 0:
                        n = n[:i]
                        break
            out[n.replace(' ', '')] = int(row['Calls'])
    return out


def main():
    line_path, stats_path = sys.argv[1:3]
    label = sys.argv[3] if len(sys.argv) > 3 else line_path
    line = None
    for text in open(line_path):
        try:
            cand = json.loads(text)
        except ValueError:
            continue
        if isinstance(cand, dict) and 'kernel_table' in cand:
            line = cand
    assert line is not None, 'no bench.py --full result line in %s' % line_path
    trace = trace_names(stats_path)
    rows = [r for r in line['kernel_table'] if r['kernel'].startswith(('gemm', 'conv_'))]
    missing = wrong = 0
    print('%s   (dtype %s, roofline kernel %s)' % (label, line.get('dtype'), line.get('roofline', {}).get('kernel')))
    print('  %-44s %8s %6s  %s' % ('kernel_table name', 'launches', 'share', 'in the trace (calls / 3 steps)'))
    for r in rows:
        calls = trace.get(r['kernel'])
        missing += calls is None
        bad = calls is not None and calls != TRACE_STEPS * r['launches']
        wrong += bad
        print('  %-44s %8d %6.4f  %s' % (r['kernel'], r['launches'], r['share'],
                                         'NO' if calls is None else 'yes (%g)%s' % (calls / TRACE_STEPS,
                                                                                   '  <- COUNT DIFFERS' if bad else '')))
    print('  -> of %d gemm / conv names, %d are not kernel names of the trace and %d have another launch count there'
          % (len(rows), missing, wrong))
    return 1 if missing or wrong else 0


if __name__ == '__main__':
    sys.exit(main())

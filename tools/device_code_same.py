#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?

    hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -Iinclude csrc/<unit>.hip -o <unit>.s     (per unit, per build)
    tools/device_code_same.py --a parent/lstm_persist.s --b lstm_persist.s front_persist.s front_stack.s

Each side is the device assembly of one or more translation units.  Per kernel symbol the tool compares the text of the
function (instructions, labels, the .amdhsa_* block, the compiler's summary comments) and the resource numbers: VGPRs, SGPRs,
LDS bytes and private-segment bytes, from the .amdhsa_* lines and from the code-object metadata.  Exit status 0 iff both
sides hold the same set of kernel symbols and every kernel is equal.

What depends on the translation unit a kernel was compiled in, or on its position there, is normalised first: the lines
that carry `.file`, `.ident` or `__hip_cuid_` are dropped, and the function-indexed local labels (.LBB<n>_<m>, BB<n>_<m> in
comments, .Lfunc_begin<n> / .Lfunc_end<n>, .Ltmp<n>) are renumbered per kernel.  Nothing else is compared or printed.
"""
import argparse
import re
import sys

DROP = ('.file', '.ident', '__hip_cuid_')
BEGIN = re.compile(r'-- Begin function (\S+)')
KERNEL = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)')
SECTION = re.compile(r'^\s*\.section\s+([^,\s]+)')
AMDHSA = {'.amdhsa_next_free_vgpr': 'vgpr', '.amdhsa_next_free_sgpr': 'sgpr',
          '.amdhsa_group_segment_fixed_size': 'lds', '.amdhsa_private_segment_fixed_size': 'private'}
META = {'.vgpr_count': 'meta_vgpr', '.sgpr_count': 'meta_sgpr', '.group_segment_fixed_size': 'meta_lds',
        '.private_segment_fixed_size': 'meta_private'}
NUMBERS = list(AMDHSA.values()) + list(META.values())


def normalise(lines):
    """function-indexed labels -> per-kernel numbering"""
    tmp = {}

    def ltmp(m):
        return '.Ltmp#%d' % tmp.setdefault(m.group(0), len(tmp))

    out = []
    for s in lines:
        s = re.sub(r'BB\d+_(\d+)', r'BB#_\1', s)
        s = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1#', s)
        s = re.sub(r'\.Ltmp\d+', ltmp, s)
        out.append(' '.join(s.split()))      # (a label's width moves the comment column behind it)
    return out


def kernels_of(path):
    """{symbol: (normalised text lines, {resource name: number})} of one assembly file"""
    with open(path) as f:
        lines = [s for s in f.read().split('\n') if not any(d in s for d in DROP)]
    blocks, cur, name = {}, None, None
    meta, in_meta, item = {}, False, None
    for i, s in enumerate(lines):
        if '.amdgpu_metadata' in s:
            in_meta = not s.strip().startswith('.end_')
            cur = None
            continue
        if in_meta:
            if re.match(r'^  - \.', s):
                item = {}
                s = '    ' + s[4:]
            m = re.match(r'^    (\.\w+):\s+(\S+)\s*$', s)
            if m and item is not None:
                if m.group(1) == '.name':
                    meta[m.group(2)] = item
                elif m.group(1) in META:
                    item[META[m.group(1)]] = int(m.group(2))
            continue
        m = BEGIN.search(s)
        if m:
            name = m.group(1)
            cur = blocks.setdefault(name, [])
            # (the .section line in front belongs to this function)
            if i > 0 and SECTION.match(lines[i - 1]):
                cur.append(lines[i - 1])
        sec = SECTION.match(s)
        if sec and cur is not None:
            nxt = lines[i + 1] if i + 1 < len(lines) else ''
            own = sec.group(1) in ('.rodata', '.AMDGPU.csdata') or (sec.group(1).startswith('.text') and not BEGIN.search(nxt))
            if not own:
                cur = None
        if cur is not None:
            cur.append(s)
    out = {}
    for name, text in blocks.items():
        if not any(KERNEL.match(s) for s in text):
            continue      # (a device function that was not inlined: part of no comparison of its own)
        nums = dict(meta.get(name, {}))
        for s in text:
            t = s.split()
            if len(t) == 2 and t[0] in AMDHSA:
                nums[AMDHSA[t[0]]] = int(t[1])
        out[name] = (normalise(text), nums)
    return out


def side(paths):
    out = {}
    for p in paths:
        for name, v in kernels_of(p).items():
            if name in out:
                sys.exit('%s: kernel %s appears twice on one side' % (p, name))
            out[name] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--a', nargs='+', required=True, metavar='FILE.s', help='device assembly of the first build')
    ap.add_argument('--b', nargs='+', required=True, metavar='FILE.s', help='device assembly of the second build')
    args = ap.parse_args()
    a, b = side(args.a), side(args.b)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print('%-9s %s' % ('only in a' if name in a else 'only in b', name))
            bad += 1
            continue
        (ta, na), (tb, nb) = a[name], b[name]
        missing = [k for k in NUMBERS if k not in na or k not in nb]
        same_text, same_nums = ta == tb, na == nb and not missing
        what = 'same' if same_text and same_nums else 'DIFFERS'
        detail = ''
        if not same_text:
            first = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
            detail += '  text: %d vs %d lines, first difference at line %d of the kernel' % (len(ta), len(tb), first + 1)
        if not same_nums:
            detail += '  numbers: %s vs %s' % (na, nb)
        print('%-9s %s  vgpr %s sgpr %s lds %s private %s%s' % (what, name, na.get('vgpr'), na.get('sgpr'), na.get('lds'),
                                                               na.get('private'), detail))
        bad += what != 'same'
    print('%d kernels in a, %d in b, %d not the same' % (len(a), len(b), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())

"""From a folder of recordings to the word store the loader reads - what the reference's preprocessing scripts do with
``librosa.load(wav, sr=8000)``, a forced alignment and HDF5 (preprocess.py:24, preprocess-fisher.py:232-250), without
librosa, h5py or an alignment of its own: segments come from a manifest.

  scan_tree(root)        entries (path, word, None, None) for root/<word>/*.wav, sorted
  read_manifest(tsv)     entries from lines  path<TAB>word[<TAB>start_s<TAB>end_s]
  build_store(entries)   read (audio.read_wav), resample to 8 kHz (audio.resample: ag_resample_poly on a GPU, float64 on
                         the host otherwise), cut, drop, stack -> (store, report)
  write_cuts(report, ..) the active stretches of build_store(trim / split) as a manifest
  save_store / load_store  one uncompressed .npz; ``dataset._open`` takes its path as ``args.dataset``

The store is a plain dict word -> float32 [n_clips, maxlen_word], zero padded: the layout preprocess-fisher.py:240-250
writes and dataset.py reads.  Samples are stored as resampled; the loader peak-normalises each pick, as the reference does.

``build_store(trim=True)`` / ``(split=True)`` find the words inside the clips by short-time energy (``audio.activity``:
ag_frame_power and ag_activity_segments on a GPU, float64 on the host otherwise): room noise before and after a word is cut
off, a long take becomes one clip per stretch, and ``write_cuts`` writes the stretches as a manifest to label by hand.

  python -m audiogan_amd.ingest (--tree DIR | --manifest TSV | --files WAV.. [--word W]) --out words.npz [--maxlen N]
         [--device D] [--trim | --split] [--top-db 40] [--floor-db -80] [--min-gap-ms 300] [--min-run-ms 50] [--pad-ms 30]
         [--cuts-out TSV]"""
import argparse
import collections
import glob
import json
import os
import sys

import numpy as np

from . import audio

DROPPED = ('silent', 'too_long', 'unreadable')


def scan_tree(root):
    """entries (path, word, None, None) for root/<word>/*.wav, sorted by word, then by file name"""
    for word in sorted(os.listdir(root)):
        d = os.path.join(root, word)
        if os.path.isdir(d):
            for path in sorted(glob.glob(os.path.join(glob.escape(d), '*.wav'))):
                yield (path, word, None, None)


def read_manifest(tsv):
    """entries from lines ``path<TAB>word[<TAB>start_s<TAB>end_s]``; ``#`` starts a comment, empty lines are skipped and a
    relative path is taken from the manifest's directory"""
    here = os.path.dirname(os.path.abspath(tsv))
    out = []
    with open(tsv, encoding='utf-8') as f:
        for no, line in enumerate(f, 1):
            line = line.split('#', 1)[0].rstrip('\r\n')
            if not line.strip():
                continue
            cols = line.split('\t')
            if len(cols) not in (2, 4):
                raise ValueError('%s:%d: path<TAB>word[<TAB>start_s<TAB>end_s], got %d columns' % (tsv, no, len(cols)))
            path = cols[0] if os.path.isabs(cols[0]) else os.path.join(here, cols[0])
            start, end = (float(cols[2]), float(cols[3])) if len(cols) == 4 else (None, None)
            out.append((path, cols[1], start, end))
    return out


def clip_length(x):
    """the loader's length rule (dataset.py:52): the index after the last non-zero sample"""
    nz = np.nonzero(x)[0]
    return int(nz[-1]) + 1 if len(nz) else 0


def _cut(start, end, n, sr):
    """the manifest's cut of a resampled file of n samples, as the slice y[int(start sr) : int(end sr)] takes it"""
    if start is None:
        return 0, n
    return slice(int(start * sr), int(end * sr)).indices(n)[:2]


def build_store(entries, out_path=None, sr=8000, maxlen=40000, device=None, rows=256, trim=False, split=False, activity=None):
    """-> (store, report).  Each file is read once; files of one (rate, channel count, sample kind) are resampled together,
    up to ``rows`` ragged rows per call of ``audio.resample``.  A segment is y[int(start_s sr) : int(end_s sr)] of the
    resampled file (preprocess-fisher.py:145-146); no bounds: the whole file.  A clip is dropped, and counted in
    report['dropped'][reason] with its path, when it is all zero ('silent'), when its length up to the last non-zero
    sample exceeds ``maxlen`` ('too_long'), or when its file cannot be read ('unreadable').  ``store``: word -> float32
    [n_clips, maxlen_word], the clips of a word in entry order; written to ``out_path`` when that is given.

    ``trim`` / ``split`` (off by default; together they behave as ``split``): ``audio.activity`` (options: the dict
    ``activity``) finds the active stretches of each entry's clip - the whole resampled file, or the manifest's cut of it; on a
    CUDA device on the resampled rows, before they leave it, and only the kept samples are copied to the host.  ``trim``: the
    clip becomes y[first start : last end], interior pauses stay.  ``split``: one clip per stretch, all under the entry's word,
    in time order.  No stretch: dropped as 'silent'; a NaN or an infinity in the clip: as 'unreadable'.  'too_long' and the
    zero-tail length rule then apply to each resulting clip.  ``report`` gains 'segments' (path -> the (start, end) samples
    of the stretches in the resampled file, per entry in entry order) and 'seconds_trimmed'."""
    entries = list(entries)
    if trim or split:
        return _build_gated(entries, out_path, sr, maxlen, device, rows, bool(split), dict(activity or {}))
    report = dict(kept={}, dropped={k: [] for k in DROPPED}, seconds_in=0.0, seconds_out=0.0, files=0)
    resampled = {}
    for part, y, counts in _resampled(entries, report, rows, sr, device):
        y = y.cpu().numpy()
        for b, p in enumerate(part):
            resampled[p] = y[b, :counts[b]].copy()
    clips = collections.OrderedDict()
    for path, word, start, end in entries:
        if path not in resampled:
            report['dropped']['unreadable'].append(path)
            continue
        y = resampled[path]
        if start is not None:
            y = y[int(start * sr):int(end * sr)]
        _add_clip(clips, report, path, word, y, maxlen, sr)
    return _stack(clips, report, out_path)


def _resampled(entries, report, rows, sr, device):
    """read each file of ``entries`` once (counted in ``report``; one that cannot be read is left out) and resample the files of
    one (rate, channel count, sample kind) together, up to ``rows`` ragged rows per call of ``audio.resample``: yields (paths,
    y [len(paths), n] on the device used, counts)"""
    files, groups = {}, collections.OrderedDict()
    for path, _, _, _ in entries:
        if path in files:
            continue
        try:
            data, rate = audio.read_wav(path)
        except (ValueError, OSError) as e:
            files[path] = e
            continue
        files[path] = (data, rate)
        report['files'] += 1
        report['seconds_in'] += data.shape[0] / float(rate)
        groups.setdefault((rate, data.shape[1], data.dtype.str), []).append(path)
    for (rate, channels, _), paths in groups.items():
        for i in range(0, len(paths), max(1, int(rows))):
            part = paths[i:i + max(1, int(rows))]
            lens = np.array([files[p][0].shape[0] for p in part], dtype=np.int64)
            batch = np.zeros((len(part), int(lens.max()), channels), dtype=files[part[0]][0].dtype)
            for b, p in enumerate(part):
                batch[b, :lens[b]] = files[p][0]
                files[p] = None
            yield (part,) + tuple(audio.resample(batch, rate, sr, lens=lens, device=device))


def _add_clip(clips, report, path, word, y, maxlen, sr):
    """the zero-tail length rule, 'silent' and 'too_long' on one clip"""
    n = clip_length(y)
    if n == 0:
        report['dropped']['silent'].append(path)
    elif n > maxlen:
        report['dropped']['too_long'].append(path)
    else:
        clips.setdefault(word, []).append(y[:n])
        report['seconds_out'] += n / float(sr)


def _stack(clips, report, out_path):
    store = {}
    for word, cs in clips.items():
        arr = np.zeros((len(cs), max(len(c) for c in cs)), dtype=np.float32)
        for i, c in enumerate(cs):
            arr[i, :len(c)] = c
        store[word] = arr
        report['kept'][word] = len(cs)
    if out_path is not None:
        save_store(store, out_path)
    return store, report


def _build_gated(entries, out_path, sr, maxlen, device, rows, split, options):
    """``build_store`` with ``trim`` or ``split``: the same reading, grouping and resampling; per batch of resampled rows the
    clips of every entry on one of its files go through ``audio.activity`` where the rows are, and what is kept is packed
    into one buffer and copied to the host once"""
    import torch
    report = dict(kept={}, dropped={k: [] for k in DROPPED}, seconds_in=0.0, seconds_out=0.0, files=0, segments={},
                  seconds_trimmed=0.0)
    users = collections.OrderedDict()          # path -> indices of the entries on it
    for i, (path, _, _, _) in enumerate(entries):
        users.setdefault(path, []).append(i)
    found = {}          # entry index -> ('unreadable' | 'silent' | None, [(start, end) in the file], [clips])
    for part, y, counts in _resampled(entries, report, rows, sr, device):
        whole, cuts = [], []          # (entry, row, offset, length)
        for b, p in enumerate(part):
            for e in users[p]:
                lo, hi = _cut(entries[e][2], entries[e][3], int(counts[b]), sr)
                (whole if entries[e][2] is None else cuts).append((e, b, lo, max(0, hi - lo)))
        segs = {}
        if whole:          # the whole files of the batch: one call on the rows as they lie
            rws = sorted(set(b for _, b, _, _ in whole))
            got = audio.activity(y[rws] if len(rws) < len(part) else y, lens=counts[rws], sr=sr, device=y.device, **options)
            at = dict(zip(rws, got))
            for e, b, _, _ in whole:
                segs[e] = at[b]
        for e, b, lo, n in cuts:
            segs[e] = audio.activity(y[b:b + 1, lo:lo + n], sr=sr, device=y.device, **options)[0] if n else \
                np.zeros((0, 2), dtype=np.int64)
        keep = []          # (entry, row, start, end), in entry and time order
        for e, b, lo, n in sorted(whole + cuts):
            sg = segs[e]
            if sg is None or not len(sg):
                found[e] = ('unreadable' if sg is None else 'silent', [], [])
                continue
            stretches = [(int(a) + lo, int(z) + lo) for a, z in sg]
            spans = stretches if split else [(stretches[0][0], stretches[-1][1])]
            found[e] = (None, stretches, [])
            report['seconds_trimmed'] += (n - sum(z - a for a, z in spans)) / float(sr)
            keep.extend((e, b, a, z) for a, z in spans)
        if keep:
            flat = torch.cat([y[b, a:z] for _, b, a, z in keep]).cpu().numpy()
            at = 0
            for e, _, a, z in keep:
                found[e][2].append(flat[at:at + z - a].copy())
                at += z - a
    clips = collections.OrderedDict()
    for e, (path, word, _, _) in enumerate(entries):
        if e not in found:
            report['dropped']['unreadable'].append(path)
            continue
        why, stretches, cs = found[e]
        report['segments'].setdefault(path, []).append(stretches)
        if why is not None:
            report['dropped'][why].append(path)
            continue
        for y in cs:
            _add_clip(clips, report, path, word, y, maxlen, sr)
    return _stack(clips, report, out_path)


def write_cuts(report, entries, tsv, sr=8000):
    """the stretches ``build_store(trim / split)`` found, as a manifest ``read_manifest`` reads: one line
    path<TAB>word<TAB>start_s<TAB>end_s per stretch, in entry and time order.  A time is '%.6f' % ((sample + 0.5) / sr):
    ``build_store`` cuts at int(start_s sr), and the half sample absorbs the rounding of the decimal text and of the
    product, so the cut gives back the sample exactly.  -> the number of lines.  Segment a long recording once
    (``--files take.wav --split --cuts-out cuts.tsv``), put the words into the second column by hand, then ``--manifest``."""
    seen, lines = {}, []
    for path, word, _, _ in entries:
        k = seen.get(path, 0)
        seen[path] = k + 1
        per_entry = report['segments'].get(path, [])
        for a, z in (per_entry[k] if k < len(per_entry) else []):
            lines.append('%s\t%s\t%.6f\t%.6f\n' % (os.path.abspath(path), word, (a + 0.5) / sr, (z + 0.5) / sr))
    with open(tsv, 'w', encoding='utf-8') as f:
        f.write('# path, word, start_s, end_s: active stretches (audiogan_amd.ingest --cuts-out)\n')
        f.writelines(lines)
    return len(lines)


def save_store(store, path):
    """one uncompressed .npz: 'words' (the keys, in order) and the array of word i under 'w<i>' - a word may hold characters
    a zip member name may not"""
    words = list(store.keys())
    arrays = {'w%d' % i: np.ascontiguousarray(store[w], dtype=np.float32) for i, w in enumerate(words)}
    with open(path, 'wb') as f:
        np.savez(f, words=np.array(words, dtype=np.str_), **arrays)


def load_store(path):
    """the whole store as a dict (an NpzFile would re-read an array at every ``dataset[key]``)"""
    with np.load(path, allow_pickle=False) as z:
        return {str(w): z['w%d' % i] for i, w in enumerate(z['words'])}


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m audiogan_amd.ingest', description=__doc__.split('\n\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--tree', help='a folder of <word>/*.wav')
    src.add_argument('--manifest', help='a TSV of path, word[, start_s, end_s]')
    src.add_argument('--files', nargs='+', metavar='WAV', help='recordings that all carry the label --word')
    ap.add_argument('--word', default='?', help="the label of --files (default '?': segment first, label the cuts by hand)")
    ap.add_argument('--out', required=True, help='the .npz to write')
    ap.add_argument('--maxlen', type=int, default=40000)
    ap.add_argument('--device', default=None)
    ap.add_argument('--trim', action='store_true', help='cut each clip to its first-to-last active stretch')
    ap.add_argument('--split', action='store_true', help='one clip per active stretch')
    ap.add_argument('--top-db', type=float, default=None, help='active: within this many dB of the loudest frame (40)')
    ap.add_argument('--floor-db', type=float, default=None, help='and above this absolute power in dB (-80)')
    ap.add_argument('--min-gap-ms', type=float, default=None, help='pauses shorter than this are closed (300)')
    ap.add_argument('--min-run-ms', type=float, default=None, help='stretches shorter than this are dropped (50)')
    ap.add_argument('--pad-ms', type=float, default=None, help='kept either side of a stretch (30)')
    ap.add_argument('--cuts-out', metavar='TSV', help='write the stretches found as a manifest (needs --trim or --split)')
    a = ap.parse_args(argv)
    if a.cuts_out and not (a.trim or a.split):
        ap.error('--cuts-out needs --trim or --split')
    if a.tree:
        entries = list(scan_tree(a.tree))
    elif a.manifest:
        entries = read_manifest(a.manifest)
    else:
        entries = [(path, a.word, None, None) for path in a.files]
    options = {k: getattr(a, k) for k in ('top_db', 'floor_db', 'min_gap_ms', 'min_run_ms', 'pad_ms') if getattr(a, k) is not None}
    if a.trim or a.split:
        store, report = build_store(entries, maxlen=a.maxlen, device=a.device, trim=a.trim, split=a.split, activity=options)
    else:
        store, report = build_store(entries, maxlen=a.maxlen, device=a.device)
    if a.cuts_out:
        write_cuts(report, entries, a.cuts_out)
    if store:
        save_store(store, a.out)
    print(json.dumps(dict(kept=report['kept'], dropped={k: len(v) for k, v in report['dropped'].items()},
                          dropped_paths=report['dropped'], seconds_in=report['seconds_in'],
                          seconds_out=report['seconds_out'],
                          **({'seconds_trimmed': report['seconds_trimmed']} if 'seconds_trimmed' in report else {})),
                     sort_keys=True))
    return 0 if store else 1


if __name__ == '__main__':
    sys.exit(main())

"""From a folder of recordings to the word store the loader reads - what the reference's preprocessing scripts do with
``librosa.load(wav, sr=8000)``, a forced alignment and HDF5 (preprocess.py:24, preprocess-fisher.py:232-250), without
librosa, h5py or a forced aligner: segments come from a manifest, from an energy gate, or from aligning a transcribed
utterance with recorded takes of its words.

  scan_tree(root)        entries (path, word, None, None) for root/<word>/*.wav, sorted
  read_manifest(tsv)     entries from lines  path<TAB>word[<TAB>start_s<TAB>end_s]
  build_store(entries)   read (audio.read_wav), resample to 8 kHz (audio.resample: ag_resample_poly on a GPU, float64 on
                         the host otherwise), cut, drop, stack -> (store, report)
  write_cuts(report, ..) the active stretches of build_store(trim / split) as a manifest
  save_store / load_store  one uncompressed .npz; ``dataset._open`` takes its path as ``args.dataset``
  read_utterances(tsv) / read_fisher_transcript(txt, wav)   transcribed utterances
  align_store(utterances, templates)   their words cut by template alignment (audiogan_amd/align.py: ag_dtw_align) -> (store,
                         report); write_word_cuts(report, tsv) writes the cuts as a manifest.  Template alignment, not an HMM
                         aligner: only words with a template are cut, and it needs a CUDA (HIP) device

The store is a plain dict word -> float32 [n_clips, maxlen_word], zero padded: the layout preprocess-fisher.py:240-250
writes and dataset.py reads.  Samples are stored as resampled; the loader peak-normalises each pick, as the reference does.

``build_store(trim=True)`` / ``(split=True)`` find the words inside the clips by short-time energy (``audio.activity``:
ag_frame_power and ag_activity_segments on a GPU, float64 on the host otherwise): room noise before and after a word is cut
off, a long take becomes one clip per stretch, and ``write_cuts`` writes the stretches as a manifest to label by hand.

  python -m audiogan_amd.ingest (--tree DIR | --manifest TSV | --files WAV.. [--word W]) --out words.npz [--maxlen N]
         [--device D] [--trim | --split] [--top-db 40] [--floor-db -80] [--min-gap-ms 300] [--min-run-ms 50] [--pad-ms 30]
         [--cuts-out TSV]
  python -m audiogan_amd.ingest --utterances TSV --templates words.npz --out words2.npz [--max-db X] [--trim]
         [--cuts-out TSV] [--maxlen N] [--device D]"""
import argparse
import collections
import glob
import json
import os
import re
import sys

import numpy as np

from . import audio

DROPPED = ('silent', 'too_long', 'unreadable', 'no_template', 'too_long_to_align')
_FILE_DROPS = DROPPED[:3]          # what ``build_store`` can report; the last two are ``align_store``'s


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
    report = dict(kept={}, dropped={k: [] for k in _FILE_DROPS}, seconds_in=0.0, seconds_out=0.0, files=0)
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
    report = dict(kept={}, dropped={k: [] for k in _FILE_DROPS}, seconds_in=0.0, seconds_out=0.0, files=0, segments={},
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


# ----------------------------------------------------------------------------------------------------------------------
# transcribed utterances: words cut by template alignment (audiogan_amd/align.py)
# ----------------------------------------------------------------------------------------------------------------------
def read_utterances(tsv):
    """entries (path, start_s, end_s, words, channel) from lines ``path<TAB>start_s<TAB>end_s<TAB>transcript[<TAB>channel]``:
    the transcript's words are separated by blanks, empty bounds mean the whole file, ``channel`` (0-based) picks one channel
    of the file instead of their mean.  ``#`` comments, empty lines and relative paths as in ``read_manifest``."""
    here = os.path.dirname(os.path.abspath(tsv))
    out = []
    with open(tsv, encoding='utf-8') as f:
        for no, line in enumerate(f, 1):
            line = line.split('#', 1)[0].rstrip('\r\n')
            if not line.strip():
                continue
            cols = line.split('\t')
            if len(cols) not in (4, 5):
                raise ValueError('%s:%d: path<TAB>start_s<TAB>end_s<TAB>transcript[<TAB>channel], got %d columns'
                                 % (tsv, no, len(cols)))
            path = cols[0] if os.path.isabs(cols[0]) else os.path.join(here, cols[0])
            start, end = (float(cols[1]), float(cols[2])) if cols[1].strip() and cols[2].strip() else (None, None)
            channel = int(cols[4]) if len(cols) == 5 and cols[4].strip() else None
            out.append((path, start, end, cols[3].split(), channel))
    return out


_NOT_WORDS = re.compile(r'\(\(.*?\)\)|\[[^\]]*\]')


def read_fisher_transcript(txt, wav_path):
    """entries as ``read_utterances`` gives them from a Fisher transcript: lines ``start end X: words`` taken apart with the
    reference's ``split(' ', 3)`` (preprocess-fisher.py:172); the speaker's first letter picks the channel of ``wav_path``
    (A: 0, B: 1).  Lines that do not parse are skipped, as there.  Words are lower-cased; ``[noise]``-style tokens and
    ``(( uncertain stretches ))`` are left out, and a line with no word left is skipped."""
    out = []
    with open(txt, encoding='utf-8', errors='replace') as f:
        for line in f:
            try:
                start, end, spk, words = line.strip().split(' ', 3)
                start, end = float(start), float(end)
                channel = {'A': 0, 'B': 1}[spk[0].upper()]
            except (ValueError, KeyError, IndexError):
                continue
            words = _NOT_WORDS.sub(' ', words.lower()).split()
            if words:
                out.append((wav_path, start, end, words, channel))
    return out


def _resampled_channels(keys, report, rows, sr, device):
    """``_resampled`` for keys (path, channel): channel None is the file as it is (the resampler takes the mean of its
    channels), a number is that channel alone, sliced HERE, on the host, so that the resampler still sees mono rows.  A key
    whose file cannot be read or lacks the channel is left out.  Yields (keys, y, counts)."""
    raw, files, groups = {}, {}, collections.OrderedDict()
    for key in keys:
        path, channel = key
        if key in files:
            continue
        if path not in raw:
            try:
                raw[path] = audio.read_wav(path)
            except (ValueError, OSError):
                raw[path] = None
                continue
            report['files'] += 1
            report['seconds_in'] += raw[path][0].shape[0] / float(raw[path][1])
        if raw[path] is None:
            continue
        data, rate = raw[path]
        if channel is not None:
            if not 0 <= channel < data.shape[1]:
                continue
            data = data[:, channel:channel + 1]
        files[key] = data
        groups.setdefault((rate, data.shape[1], data.dtype.str), []).append(key)
    for (rate, channels, _), ks in groups.items():
        for i in range(0, len(ks), max(1, int(rows))):
            part = ks[i:i + max(1, int(rows))]
            lens = np.array([files[k].shape[0] for k in part], dtype=np.int64)
            batch = np.zeros((len(part), int(lens.max()), channels), dtype=files[part[0]].dtype)
            for b, k in enumerate(part):
                batch[b, :lens[b]] = files[k]
                files[k] = None
            yield (part,) + tuple(audio.resample(batch, rate, sr, lens=lens, device=device))


def align_store(utterances, templates, out_path=None, sr=8000, maxlen=40000, device=None, rows=256, max_db=None, trim=False,
                activity=None):
    """``utterances``: entries of ``read_utterances`` / ``read_fisher_transcript``; ``templates``: word -> cepstral rows
    (``align.pick_templates`` on a store of isolated or hand-labelled words) -> (store, report) as ``build_store`` gives them.
    Every file (channel) is read and resampled once, each utterance y[int(start_s sr) : int(end_s sr)] goes through
    ``align.align_utterances`` and every word of its transcript becomes one clip under that word, in utterance and time order.
    An utterance is dropped whole, with its path in report['dropped'][reason], when a word of it has no template
    ('no_template'; the words are counted in report['missing_words']), when it or its reference exceeds 1024 frames
    ('too_long_to_align') or when its file cannot be read ('unreadable').  ``max_db``: a cut whose aligned distance to its
    template exceeds it is dropped as 'poor_match'.  ``trim``: each cut is narrowed to its first-to-last active stretch
    (``audio.activity``, options ``activity``).  'silent' and 'too_long' then apply per clip.  report['cuts']: (path, word,
    start, end, db) of every clip handed to the store, samples of the resampled file - ``write_word_cuts`` writes them.
    Needs a CUDA (HIP) device (``align.require_device``)."""
    import torch
    from . import align
    utterances = list(utterances)
    device = align.require_device(device)
    report = dict(kept={}, dropped={k: [] for k in DROPPED}, seconds_in=0.0, seconds_out=0.0, files=0, cuts=[],
                  missing_words={})
    if max_db is not None:
        report['dropped']['poor_match'] = []
    options = dict(activity or {})
    found = {}          # utterance index -> [(word, start, end, db, samples)] | reason
    keys = [(u[0], u[4]) for u in utterances]
    for part, y, counts in _resampled_channels(keys, report, rows, sr, device):
        yh = y.cpu().numpy()
        mine = [(e, b) + _cut(utterances[e][1], utterances[e][2], int(counts[b]), sr)
                for b, k in enumerate(part) for e in range(len(utterances)) if keys[e] == k]
        if not mine:
            continue
        ln = np.array([max(0, hi - lo) for _, _, lo, hi in mine], dtype=np.int64)
        waves = np.zeros((len(mine), max(1, int(ln.max()))), dtype=np.float32)
        for r, (_, b, lo, _) in enumerate(mine):
            waves[r, :ln[r]] = yh[b, lo:lo + ln[r]]
        got = align.align_utterances(torch.from_numpy(waves), ln, [utterances[e][3] for e, _, _, _ in mine], templates,
                                     device=device)
        for r, (e, _, lo, _) in enumerate(mine):
            if got[r]['dropped'] is not None:
                found[e] = got[r]['dropped']
                continue
            found[e] = [(w, lo + a, lo + z, db, waves[r, a:z]) for w, a, z, db in got[r]['cuts']]
    clips = collections.OrderedDict()
    for e, (path, _, _, words, _) in enumerate(utterances):
        if e not in found:
            report['dropped']['unreadable'].append(path)
            continue
        if isinstance(found[e], tuple):
            reason, detail = found[e]
            report['dropped'][reason].append(path)
            if reason == 'no_template':
                for w in dict.fromkeys(w for w in words if w not in templates):
                    report['missing_words'][w] = report['missing_words'].get(w, 0) + 1
            continue
        cuts = found[e]
        if trim and cuts:
            cl = np.array([len(c[4]) for c in cuts], dtype=np.int64)
            buf = np.zeros((len(cuts), max(1, int(cl.max()))), dtype=np.float32)
            for r, c in enumerate(cuts):
                buf[r, :cl[r]] = c[4]
            segs = audio.activity(buf, lens=cl, sr=sr, device=device, **options)
        for r, (w, a, z, db, x) in enumerate(cuts):
            if max_db is not None and db > max_db:
                report['dropped']['poor_match'].append(path)
                continue
            if trim:
                if segs[r] is None or not len(segs[r]):
                    report['dropped']['unreadable' if segs[r] is None else 'silent'].append(path)
                    continue
                a, z, x = a + int(segs[r][0][0]), a + int(segs[r][-1][1]), x[int(segs[r][0][0]):int(segs[r][-1][1])]
            report['cuts'].append((path, w, a, z, db))
            _add_clip(clips, report, path, w, x, maxlen, sr)
    return _stack(clips, report, out_path)


def write_word_cuts(report, tsv, sr=8000):
    """report['cuts'] of ``align_store`` as a manifest ``read_manifest`` reads, one line per clip with ``write_cuts``' time rule
    (a time is '%.6f' % ((sample + 0.5) / sr), which ``build_store`` cuts back to the sample exactly): ``--manifest`` on it
    builds the same store from files whose entries named no channel.  -> the number of lines."""
    with open(tsv, 'w', encoding='utf-8') as f:
        f.write('# path, word, start_s, end_s: words cut by template alignment (audiogan_amd.ingest --utterances)\n')
        for path, word, a, z, _ in report['cuts']:
            f.write('%s\t%s\t%.6f\t%.6f\n' % (os.path.abspath(path), word, (a + 0.5) / sr, (z + 0.5) / sr))
    return len(report['cuts'])


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


def _main_utterances(ap, a):
    """``--utterances``: templates from the store ``--templates``, ``align_store``, the same JSON line as the other sources"""
    from . import align
    if not a.templates:
        ap.error('--utterances needs --templates')
    if a.split:
        ap.error('--split does not go with --utterances')
    try:
        device = align.require_device(a.device)
    except RuntimeError as e:
        print(str(e), file=sys.stderr)
        return 2
    utterances = read_utterances(a.utterances)
    templates = align.pick_templates(load_store(a.templates), [w for u in utterances for w in u[3]], device=device)
    options = {k: getattr(a, k) for k in ('top_db', 'floor_db', 'min_gap_ms', 'min_run_ms', 'pad_ms') if getattr(a, k) is not None}
    store, report = align_store(utterances, templates, maxlen=a.maxlen, device=device, max_db=a.max_db, trim=a.trim,
                                activity=options)
    if a.cuts_out:
        write_word_cuts(report, a.cuts_out)
    if store:
        save_store(store, a.out)
    print(json.dumps(dict(kept=report['kept'], dropped={k: len(v) for k, v in report['dropped'].items()},
                          dropped_paths=report['dropped'], missing_words=report['missing_words'],
                          seconds_in=report['seconds_in'], seconds_out=report['seconds_out']), sort_keys=True))
    return 0 if store else 1


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
    src.add_argument('--utterances', metavar='TSV', help='a TSV of path, start_s, end_s, transcript[, channel]: cut the words '
                     'by template alignment (needs --templates and a CUDA (HIP) device)')
    ap.add_argument('--templates', metavar='NPZ', help='with --utterances: a word store whose clips supply the templates')
    ap.add_argument('--max-db', type=float, default=None, help='with --utterances: drop cuts further than this from their '
                    'template, in dB of aligned mel-cepstral distance (default: keep all)')
    a = ap.parse_args(argv)
    if a.utterances:
        return _main_utterances(ap, a)
    if a.templates or a.max_db is not None:
        ap.error('--templates and --max-db go with --utterances')
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

#!/usr/bin/env python3
# -*- coding:utf-8 -*-
"""Average cost Cavg of a language-recognition score file on an MI355X - command-line compatible with the reference's
computeCavg.py (`computeCavg.py -pairs|-matrix <trials> <scores>`, prints `Cavg <value rounded to 4 decimals>`; called by
score/metric/getCavg.sh for scoreSets.sh --metric Cavg).  The reference script is Python 2; this one runs on Python 3.

    trials:          <lang> <utt> <target|nontarget>
    scores, -pairs:  <lang> <utt> <score>
    scores, -matrix: a first row of language names, then <utt> <score of language 1> <score of language 2> ...

Language ids are the ranks of the sorted language names of the trials file; an utterance's own language comes from its
`target` line, an utterance without one is unknown (-1).  Scored pairs that the trials file does not list are dropped.
The text is parsed here; the scores go to the device as float32 and libasv_amd.so counts them (asv_cavg).  There is no
CPU path: without a ROCm device or the library this exits non-zero.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "pytorch"))

BINS = 20
P_TARGET = 0.5


def read_trials(path):
    """-> (lang2id, utt2lang_id, listed): ids by sorted language name, the language id of every utterance with a `target` line,
    the set of (lang, utt) pairs of the file."""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if len(parts) != 3:
                raise ValueError("%s:%d: expected '<lang> <utt> <target|nontarget>', got %r" % (path, n, line.rstrip("\n")))
            rows.append(parts)
    lang2id = {lang: i for i, lang in enumerate(sorted({r[0] for r in rows}))}
    utt2lang_id = {utt: lang2id[lang] for lang, utt, target in rows if target == "target"}
    return lang2id, utt2lang_id, {(lang, utt) for lang, utt, _ in rows}


def _arrays(triples):
    model = np.asarray([t[0] for t in triples], dtype=np.int32)
    true = np.asarray([t[1] for t in triples], dtype=np.int32)
    return model, true, np.asarray([t[2] for t in triples], dtype=np.float64)


def read_pair_scores(path, lang2id, utt2lang_id, listed):
    """-> (model_lang int32 [n], true_lang int32 [n] (-1 unknown), scores float64 [n]) in file order."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if len(parts) != 3:
                raise ValueError("%s:%d: expected '<lang> <utt> <score>', got %r" % (path, n, line.rstrip("\n")))
            lang, utt, score = parts
            if (lang, utt) in listed:
                out.append((lang2id[lang], utt2lang_id.get(utt, -1), float(score)))
    return _arrays(out)


def read_matrix_scores(path, lang2id, utt2lang_id, listed):
    """The matrix form as the same pair arrays: row by row, within a row in the order of the header's languages."""
    out = []
    with open(path) as f:
        header = f.readline().split()
        for n, line in enumerate(f, 2):
            parts = line.split()
            if len(parts) != len(header) + 1:
                raise ValueError("%s:%d: expected an utterance and %d scores, got %d fields" % (path, n, len(header), len(parts)))
            utt = parts[0]
            for lang, score in zip(header, parts[1:]):
                if (lang, utt) in listed:
                    out.append((lang2id[lang], utt2lang_id.get(utt, -1), float(score)))
    return _arrays(out)


def main(argv=None, scoring=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 3 or argv[0] not in ("-pairs", "-matrix"):
        print("usage: computeCavg.py [-pairs|-matrix] trials scores")
        return 0
    form, trials, scores = argv
    lang2id, utt2lang_id, listed = read_trials(trials)
    reader = read_pair_scores if form == "-pairs" else read_matrix_scores
    model, true, values = reader(scores, lang2id, utt2lang_id, listed)
    if values.size == 0:
        raise ValueError("%s: no scored pair is listed in %s" % (scores, trials))
    if scoring is None:
        from libs.amd import scoring
    min_cavg, _ = scoring.cavg(values.astype(np.float32), model, true, len(lang2id), bins=BINS, p_target=P_TARGET)
    print("Cavg", round(min_cavg, 4))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Test-only numpy restatement of the row front end the caption-metric kernels share (RowNgrams, csrc/ngram.hpp), and the device
tables as numpy arrays.  The emulators of the three kernels (`emul_cider_d` in tests/test_cider_device_host.py,
`candidate_vectors` in tests/emul_consensus.py, `emul_caption_metrics` in tests/test_caption_metrics_host.py) build on it."""
import collections

import numpy as np

from dlsg_amd import scoring as S

NONE = S.NGRAM_NONE
TABLES = ('gram_keys', 'gram_idf', 'clip_off', 'ref_off', 'ref_norm', 'ref_len', 'ent_keys', 'ent_w', 'ref_words')

RowNgrams = collections.namedtuple('RowNgrams', 'ln bad code keys kbad first tf')


def row_ngrams(row, end_id, V, k):
    """the order-(k + 1) n-grams of one id row: ln the words before the first end_id (all without one); per word `bad` (an id
    outside [0, V)) and its 16-bit `code` (NONE when bad); per position i < max(ln - k, 0) the packed key `keys[i]`, `kbad[i]`
    (a bad word among its k + 1), `first[i]` (no equal key before it, whatever kbad is) and the key's count `tf[i]`"""
    row = np.asarray(row)
    hits = np.nonzero(row == end_id)[0]
    ln = int(hits[0]) if len(hits) else len(row)
    words = row[:ln]
    bad = (words < 0) | (words >= V)
    code = np.where(bad, NONE, words).astype(np.int64)
    m = max(ln - k, 0)
    keys = [S.pack_ngram([int(x) for x in code[i:i + k + 1]]) for i in range(m)]
    kbad = [bool(bad[i:i + k + 1].any()) for i in range(m)]
    first = [keys.index(keys[i]) == i for i in range(m)]
    tf = [keys.count(keys[i]) for i in range(m)]
    return RowNgrams(ln, bad, code, keys, kbad, first, tf)


def np_tables(tb):
    """the device tables of a scoring.DeviceCiderD or DeviceCaptionMetrics as numpy arrays by name: n-gram keys as uint64,
    reference words as int64 codes"""
    a = {k: getattr(tb, k).cpu().numpy() for k in TABLES if k in vars(tb)}
    for k in ('gram_keys', 'ent_keys'):
        if k in a:
            a[k] = a[k].view(np.uint64)
    if 'ref_words' in a:
        a['ref_words'] = a['ref_words'].view(np.uint16).astype(np.int64)
    return a


def find(keys, key):
    """index of `key` in the sorted uint64 array `keys`, -1 if absent"""
    p = int(np.searchsorted(keys, np.uint64(key)))
    return p if p < len(keys) and keys[p] == np.uint64(key) else -1

"""Test-only restatement of the consensus kernel (dlsg_cider_consensus, csrc/cider.hip) in numpy float64, on id rows and the
device tables of `scoring.DeviceCiderD`: per candidate the packed n-gram keys at every position, kept at their first position
with their count, idf by a search in the corpus table (log_n when absent and for a key that holds an id outside [0, V), which
is never looked up but does match itself); per ordered pair the clipped products, the norms, the length penalty; weights,
expected utilities in index order, ranks by counting.  `ConsensusEmul` binds it as `ops.cider_consensus` on top of the beam
emulators and tests/test_scst_host.py's ScstEmul (sampling, and the record of op names)."""
import math

import numpy as np
import torch

from dlsg_amd import scoring as S
from emul_groups import GroupsEmul
from emul_ngram import find as _find, row_ngrams
from test_scst_host import ScstEmul


def candidate_vectors(tb, gram_keys, gram_idf, row, end_id):
    """phase A for one id row: ([per order {key: weight} in first-position order], [norm per order], bigram count)"""
    n, ln = tb.n, 0
    vecs, norms = [], []
    for k in range(n):
        ln, _, _, keys, kbad, first, tf = row_ngrams(row, end_id, tb.V, k)
        vec = {}
        for i in range(len(keys)):
            if not first[i]:
                continue
            p = -1 if kbad[i] else _find(gram_keys, keys[i])
            vec[keys[i]] = tf[i] * (gram_idf[p] if p >= 0 else tb.log_n)
        vecs.append(vec)
        norms.append(math.sqrt(sum(w * w for w in vec.values())))
    return vecs, norms, (max(ln - 1, 0) if n >= 2 else 0)


def emul_cider_consensus(tb, ids, end_id, scores=None, temperature=1.0):
    """(util (B, n, n), expected (B, n), order (B, n)) as numpy arrays"""
    gram_keys = tb.gram_keys.cpu().numpy().view(np.uint64)
    gram_idf = tb.gram_idf.cpu().numpy()
    ids = ids.cpu().numpy()
    B, n, L = ids.shape
    assert 1 <= n <= 32 and 1 <= L <= 64 and temperature > 0.0
    util = np.zeros((B, n, n), dtype=np.float64)
    expected = np.zeros((B, n), dtype=np.float64)
    order = np.zeros((B, n), dtype=np.int64)
    two_s2 = 2.0 * (tb.sigma * tb.sigma)
    for b in range(B):
        cand = [candidate_vectors(tb, gram_keys, gram_idf, ids[b, i], end_id) for i in range(n)]
        for i, (vi, ni, li) in enumerate(cand):
            for j, (vj, nj, lj) in enumerate(cand):
                pen = math.exp(-float(li - lj) ** 2 / two_s2)
                s = 0.0
                for k in range(tb.n):
                    v = sum(min(w, vj[k].get(key, 0.0)) * vj[k].get(key, 0.0) for key, w in vi[k].items())
                    if ni[k] != 0.0 and nj[k] != 0.0:
                        v /= ni[k] * nj[k]
                    s += v * pen
                util[b, i, j] = s / tb.n * 10.0
        q = S.consensus_weights(None if scores is None else scores[b].cpu().numpy(), n, temperature)
        for i in range(n):
            if q[i] < 0.0:
                expected[b, i] = -np.inf
                continue
            num = den = 0.0
            for j in range(n):
                if j != i and q[j] > 0.0:
                    num += q[j] * util[b, i, j]
                    den += q[j]
            expected[b, i] = num / den if den > 0.0 else 0.0
        for i in range(n):
            e = expected[b, i]
            rank = sum(1 for j in range(n) if expected[b, j] > e or (expected[b, j] == e and j < i))
            order[b, rank] = i
    return util, expected, order


class ConsensusEmul(GroupsEmul, ScstEmul):
    """the beam emulators and the sampler's + `cider_consensus`; `recording` as in ScstEmul"""

    def cider_consensus(self, ids, end_id, tables, scores, temperature, util, expected, order):
        assert ids.dtype == torch.int64 and ids.dim() == 3 and expected.dtype == torch.float64 and order.dtype == torch.int64
        assert scores is None or scores.dtype == torch.float32
        u, e, o = emul_cider_consensus(tables, ids, end_id, scores, temperature)
        if util is not None:
            util.copy_(torch.from_numpy(u))
        expected.copy_(torch.from_numpy(e))
        order.copy_(torch.from_numpy(o))

"""caption scoring and the evaluation driver (reference evaluate.py:16-98 and the pure-Python
metrics of caption-eval/pycocoevalcap: BLEU-1..4, ROUGE_L, CIDEr-D).  CPU-side, off the GPU critical path, except for
`DeviceCiderD`: the self-critical reward scored on the GPU (`dlsg_cider_d`) against tables built from `CiderD`'s, and for
`DeviceCaptionMetrics` / `DeviceMixedReward`: sentence BLEU-1..4 and ROUGE_L on the GPU (`dlsg_caption_metrics`) and their
weighted mix with CIDEr-D as the reward.

Not reproduced: METEOR and the Stanford PTB tokenizer (caption-eval/pycocoevalcap/{meteor,tokenizer}) shell out to Java with
jars that are not in the reference tree; `tokenize` below is a regular-expression stand-in that lower-cases, splits
punctuation off and drops the tokenizer's punctuation list (ptbtokenizer.py:21-22), which is exact for the model's own
output (space-joined vocabulary words) and close for the raw reference sentences.

The metric definitions follow the published coco-caption algorithms:
  BLEU    corpus-level modified n-gram precision, brevity penalty against the CLOSEST reference length (bleu.py:40)
  ROUGE_L F-measure (beta = 1.2) of the best LCS precision and the best LCS recall over the references (rouge.py:43-71)
  CIDEr-D mean over n = 1..4 of clipped tf-idf cosine similarity with a Gaussian length penalty (sigma = 6), x10,
          idf from the evaluated reference set itself (cider_scorer.py:106-180)
pinned by tests/golden/scoring.json, produced by the reference's own scorer classes.
"""
import collections
import math
import re

import numpy as np

PUNCTUATIONS = frozenset(["''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...", ";"])
_TOKEN = re.compile(r"\.\.\.|--|``|''|[A-Za-z0-9]+(?:'[a-z]+)?|[^\sA-Za-z0-9]")


def tokenize(sentence):
    """lower-cased tokens without punctuation, joined by single spaces"""
    return ' '.join(t for t in _TOKEN.findall(sentence.lower().replace('\n', ' ')) if t not in PUNCTUATIONS)


def _ngrams(words, n):
    c = collections.Counter()
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            c[tuple(words[i:i + k])] += 1
    return c


# ------------------------------------------------------------------------------------------------ BLEU
def bleu(gts, res, n=4):
    """gts: id -> list of tokenized references; res: id -> [tokenized hypothesis].  Returns ([BLEU_1..n], per-id lists)."""
    small, tiny = 1e-9, 1e-15
    ids = sorted(gts.keys())
    tot_guess, tot_correct = [0] * n, [0] * n
    tot_test = tot_ref = 0
    per = [[] for _ in range(n)]
    for i in ids:
        hyp = res[i][0].split()
        refs = [r.split() for r in gts[i]]
        hc = _ngrams(hyp, n)
        mx = collections.Counter()
        for r in refs:
            for g, c in _ngrams(r, n).items():
                if c > mx[g]:
                    mx[g] = c
        guess = [max(0, len(hyp) - k) for k in range(n)]
        correct = [0] * n
        for g, c in hc.items():
            correct[len(g) - 1] += min(c, mx.get(g, 0))
        reflen = min((abs(len(r) - len(hyp)), len(r)) for r in refs)[1]            # closest length, shorter on ties
        tot_test += len(hyp); tot_ref += reflen
        b = 1.0
        ratio = (len(hyp) + tiny) / (reflen + small)
        for k in range(n):
            tot_guess[k] += guess[k]; tot_correct[k] += correct[k]
            b *= (correct[k] + tiny) / (guess[k] + small)
            s = b ** (1.0 / (k + 1))
            per[k].append(s * math.exp(1 - 1 / ratio) if ratio < 1 else s)
    out, b = [], 1.0
    ratio = (tot_test + tiny) / (tot_ref + small)
    for k in range(n):
        b *= (tot_correct[k] + tiny) / (tot_guess[k] + small)
        s = b ** (1.0 / (k + 1))
        out.append(s * math.exp(1 - 1 / ratio) if ratio < 1 else s)
    return out, per


# ------------------------------------------------------------------------------------------------ ROUGE_L
def _lcs(a, b):
    if len(a) < len(b):
        a, b = b, a
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b, 1):
            cur.append(prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[len(b)]


def rouge_l(gts, res, beta=1.2):
    ids = sorted(gts.keys())
    per = []
    for i in ids:
        hyp = res[i][0].split(' ')
        p = r = 0.0
        for ref in gts[i]:
            rt = ref.split(' ')
            l = _lcs(rt, hyp)
            p, r = max(p, l / float(len(hyp))), max(r, l / float(len(rt)))
        per.append((1 + beta ** 2) * p * r / (r + beta ** 2 * p) if p and r else 0.0)
    return sum(per) / len(per), per


# ------------------------------------------------------------------------------------------------ CIDEr-D
def cider(gts, res, n=4, sigma=6.0):
    ids = sorted(gts.keys())
    hyp = [_ngrams(res[i][0].split(), n) for i in ids]
    refs = [[_ngrams(r.split(), n) for r in gts[i]] for i in ids]
    df = collections.Counter()
    for rs in refs:
        for g in set(g for r in rs for g in r):
            df[g] += 1
    log_n = math.log(float(len(ids)))

    def vec(cnt):
        v = [dict() for _ in range(n)]
        norm = [0.0] * n
        length = 0
        for g, tf in cnt.items():
            k = len(g) - 1
            w = float(tf) * (log_n - math.log(max(1.0, df.get(g, 0.0))))
            v[k][g] = w
            norm[k] += w * w
            if k == 1:
                length += tf               # the reference scorer counts BIGRAMS here (cider_scorer.py:125-126)
        return v, [math.sqrt(x) for x in norm], length
    per = []
    for h, rs in zip(hyp, refs):
        vh, nh, lh = vec(h)
        tot = [0.0] * n
        for r in rs:
            vr, nr, lr = vec(r)
            pen = math.e ** (-(float(lh - lr) ** 2) / (2 * sigma ** 2))
            for k in range(n):
                s = sum(min(w, vr[k].get(g, 0.0)) * vr[k].get(g, 0.0) for g, w in vh[k].items())
                if nh[k] != 0 and nr[k] != 0:
                    s /= nh[k] * nr[k]
                tot[k] += s * pen
        per.append(sum(tot) / n / len(rs) * 10.0)
    return sum(per) / len(per), per


class CiderD(object):
    """CIDEr-D as a reward (self-critical training): `refs` {vid: [tokenized caption, ...]} is the training corpus; document
    frequencies, log N and every reference's tf-idf vectors are computed once here, so `scores` only vectorises the hypotheses.
    Same arithmetic as `cider` (clipping, sigma = 6 length penalty, x10): with the corpus equal to the scored set,
    scores(sorted ids, hyps) == cider(gts, res)[1]."""

    def __init__(self, refs, n=4, sigma=6.0):
        self.n, self.sigma = n, sigma
        grams = {v: [_ngrams(r.split(), n) for r in refs[v]] for v in sorted(refs)}
        df = collections.Counter()
        for rs in grams.values():
            for g in set(g for r in rs for g in r):
                df[g] += 1
        self.df = df
        self.log_n = math.log(float(len(grams)))
        self.ref_vecs = {v: [self._vec(r) for r in rs] for v, rs in grams.items()}

    def _vec(self, cnt):
        n, df, log_n = self.n, self.df, self.log_n
        v = [dict() for _ in range(n)]
        norm = [0.0] * n
        length = 0
        for g, tf in cnt.items():
            k = len(g) - 1
            w = float(tf) * (log_n - math.log(max(1.0, df.get(g, 0.0))))
            v[k][g] = w
            norm[k] += w * w
            if k == 1:
                length += tf               # bigrams, as in `cider`
        return v, [math.sqrt(x) for x in norm], length

    def _score(self, vid, hyp):
        n, sigma = self.n, self.sigma
        vh, nh, lh = self._vec(_ngrams(hyp.split(), n))
        rs = self.ref_vecs[vid]
        tot = [0.0] * n
        for vr, nr, lr in rs:
            pen = math.e ** (-(float(lh - lr) ** 2) / (2 * sigma ** 2))
            for k in range(n):
                s = sum(min(w, vr[k].get(g, 0.0)) * vr[k].get(g, 0.0) for g, w in vh[k].items())
                if nh[k] != 0 and nr[k] != 0:
                    s /= nh[k] * nr[k]
                tot[k] += s * pen
        return sum(tot) / n / len(rs) * 10.0

    def scores(self, vids, hyps):
        """CIDEr-D of hyps[i] (tokenized, space-joined) against the references of vids[i] -> float64 array.  A (vid, caption)
        pair that repeats within the call (n samples of a clip often agree) is scored once."""
        memo = {}
        out = np.empty(len(hyps), dtype=np.float64)
        for i, (v, h) in enumerate(zip(vids, hyps)):
            key = (v, h)
            if key not in memo:
                memo[key] = self._score(v, h)
            out[i] = memo[key]
        return out

    def pairwise(self, hyps):
        """U (n, n) float64 of one clip's candidate captions (tokenized strings) against each other: U[i][j] is what `_score`
        gives hyps[i] when hyps[j] is the clip's only reference, on the corpus idf.  Not symmetric (the clipping)."""
        n, sigma = self.n, self.sigma
        vecs = [self._vec(_ngrams(h.split(), n)) for h in hyps]
        U = np.zeros((len(hyps), len(hyps)), dtype=np.float64)
        for i, (vh, nh, lh) in enumerate(vecs):
            for j, (vr, nr, lr) in enumerate(vecs):
                pen = math.e ** (-(float(lh - lr) ** 2) / (2 * sigma ** 2))
                tot = 0.0
                for k in range(n):
                    s = sum(min(w, vr[k].get(g, 0.0)) * vr[k].get(g, 0.0) for g, w in vh[k].items())
                    if nh[k] != 0 and nr[k] != 0:
                        s /= nh[k] * nr[k]
                    tot += s * pen
                U[i, j] = tot / n * 10.0
        return U

    def consensus(self, hyps, scores=None, temperature=1.0):
        """Consensus (minimum Bayes risk) ranking of one clip's candidates: (order, expected).  expected[i] is the mean of
        U[i][j] = `pairwise(hyps)` over the OTHER candidates j, weighted q_j = exp((scores[j] - max valid score) / temperature)
        (scores None: 1); a candidate whose score is -inf or NaN is invalid: weight 0, expected -inf.  0 where no other candidate
        has weight.  order sorts expected descending, ties to the lower index (int64).  The host form of
        `DeviceCiderD.consensus_device`."""
        if not temperature > 0.0:
            raise ValueError('consensus temperature %r must be positive' % (temperature,))
        U = self.pairwise(hyps)
        q = consensus_weights(scores, len(hyps), temperature)
        expected = np.full(len(hyps), -np.inf, dtype=np.float64)
        for i in range(len(hyps)):
            if q[i] < 0.0:
                continue
            num = den = 0.0
            for j in range(len(hyps)):
                if j != i and q[j] > 0.0:
                    num += q[j] * U[i, j]
                    den += q[j]
            expected[i] = num / den if den > 0.0 else 0.0
        order = np.array(sorted(range(len(hyps)), key=lambda i: (-expected[i], i)), dtype=np.int64)
        return order, expected

    def to_device(self, vocab, device='cuda'):
        """the same scorer with device tables over `vocab`'s ids (`DeviceCiderD`); the corpus statistics are not recomputed"""
        return DeviceCiderD(None, vocab, self.n, self.sigma, device, _cider=self)


MAX_CANDIDATES, MAX_CANDIDATE_WORDS = 32, 64        # limits of dlsg_cider_consensus


def consensus_weights(scores, n, temperature):
    """the weights of `dlsg_cider_consensus` as a float64 array: 1 without scores, else exp((s - max valid s) / temperature) on
    the float32 scores, -1 for an invalid (-inf or NaN) one; temperature inf weighs every valid candidate 1"""
    if scores is None:
        return np.ones(n, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float32).astype(np.float64).reshape(n)
    valid = s > -np.inf                                              # (a NaN fails the comparison)
    q = np.full(n, -1.0, dtype=np.float64)
    if valid.any():
        mx = s[valid].max()
        for j in np.nonzero(valid)[0]:
            q[j] = 1.0 if s[j] == mx or math.isinf(temperature) else math.exp((s[j] - mx) / temperature)
    return q


NGRAM_NONE = 0xFFFF             # the key slot of a position past the n-gram's order (and the bound on the vocabulary size)


def pack_ngram(ids):
    """the 64-bit key of an n-gram of word ids (n <= 4): sum_j s_j << 16 j, s_j = ids[j] for j < n, NGRAM_NONE past it"""
    key = 0
    for j in range(4):
        key |= (ids[j] if j < len(ids) else NGRAM_NONE) << (16 * j)
    return key


class DeviceCiderD(object):
    """CIDEr-D of captions given as vocabulary ids, scored on the GPU (`dlsg_cider_d`): the self-critical reward without a trip
    through the host.  The corpus statistics are those of `CiderD(refs, n, sigma)`, built once on the host and copied to HBM:
      * the corpus n-gram table -- every n-gram of the references made only of in-vocabulary words (`vocab.word2idx`: no
        `<unk>` mapping, so an out-of-vocabulary reference word never meets a sampled `<unk>`), keyed by `pack_ngram`, sorted,
        with its idf log_n - log(max(1, df)) (float64);
      * the references -- per reference its in-vocabulary n-grams (sorted keys, tf-idf weights), its n norms and its length
        (bigram count), the norms and lengths being CiderD's own, out-of-vocabulary n-grams included; CSR offsets from clip to
        references (clips in sorted vid order) and from reference to entries.
    `scores_device(ids, clip_idx)` scores id rows with decode_tokens' rule (the words before the first <end>) and gives what
    `CiderD.scores` gives for the decoded strings (to rounding, 1e-12); an id outside [0, len(vocab)) is a word that matches no
    reference.  `scores(vids, hyps)` (strings) is the host CiderD's, so this object serves wherever a CiderD does.
    `ops`: the kernel binding (None: a `hip.HipOps` made on first use)."""

    def __init__(self, refs, vocab, n=4, sigma=6.0, device='cuda', _cider=None):
        import torch
        V = len(vocab)
        if V > NGRAM_NONE:
            raise ValueError('DeviceCiderD packs 16 bits per word: a vocabulary of %d words is over the %d limit' % (V, NGRAM_NONE))
        if not 1 <= int(n) <= 4:
            raise ValueError('DeviceCiderD scores n-grams of orders 1..n with n <= 4, not n = %r' % (n,))
        cd = _cider if _cider is not None else CiderD(refs, n, sigma)
        self.cider, self.vocab, self.device = cd, vocab, torch.device(device)
        self.n, self.sigma, self.V, self.log_n = int(cd.n), float(cd.sigma), V, float(cd.log_n)
        self.end_id = vocab('<end>')
        self.ops = None
        w2i = vocab.word2idx
        keyof = {}

        def key(g):
            k = keyof.get(g, False)
            if k is False:
                ids = [w2i.get(w) for w in g]
                k = keyof[g] = None if any(i is None for i in ids) else pack_ngram(ids)
            return k
        gk, gi = [], []
        for g, d in cd.df.items():
            k = key(g)
            if k is not None:
                gk.append(k)
                gi.append(cd.log_n - math.log(max(1.0, d)))
        gk = np.array(gk, dtype=np.uint64)
        order = np.argsort(gk, kind='stable')
        self.vids = sorted(cd.ref_vecs)
        self.vid_index = {v: i for i, v in enumerate(self.vids)}
        clip_off, norms, lens, ent_ref, ek, ew = [0], [], [], [], [], []
        q = 0
        for v in self.vids:
            for vr, nr, lr in cd.ref_vecs[v]:
                for k in range(self.n):
                    for g, w in vr[k].items():
                        kk = key(g)
                        if kk is not None:
                            ent_ref.append(q)
                            ek.append(kk)
                            ew.append(w)
                norms.append(list(nr) + [0.0] * (4 - len(nr)))
                lens.append(lr)
                q += 1
            clip_off.append(q)
        ek, ent_ref = np.array(ek, dtype=np.uint64), np.array(ent_ref, dtype=np.int64)
        eo = np.lexsort((ek, ent_ref))                               # by reference, then by key
        ref_off = np.zeros(q + 1, dtype=np.int64)
        np.cumsum(np.bincount(ent_ref, minlength=q), out=ref_off[1:])

        def dev(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.device)
        self.gram_keys = dev(gk[order].view(np.int64), torch.int64)  # uint64 bits
        self.gram_idf = dev(np.array(gi, dtype=np.float64)[order], torch.float64)
        self.clip_off = dev(np.array(clip_off, dtype=np.int64), torch.int64)
        self.ref_off = dev(ref_off, torch.int64)
        self.ref_norm = dev(np.array(norms, dtype=np.float64).reshape(q, 4), torch.float64)
        self.ref_len = dev(np.array(lens, dtype=np.int32), torch.int32)
        self.ent_keys = dev(ek[eo].view(np.int64), torch.int64)
        self.ent_w = dev(np.array(ew, dtype=np.float64)[eo], torch.float64)
        self.n_clips = len(self.vids)

    def __getattr__(self, name):                                     # df, log_n, ref_vecs, ...: the host scorer's
        if name == 'cider':
            raise AttributeError(name)
        return getattr(self.cider, name)

    def scores(self, vids, hyps):
        """CiderD.scores: tokenized strings on the host"""
        return self.cider.scores(vids, hyps)

    def index(self, vids):
        """clip indices of `vids` (int32 tensor on the tables' device, one asynchronous host-to-device copy); KeyError for a vid
        outside the corpus"""
        import torch
        from .hip import host_to_device
        return host_to_device(np.array([self.vid_index[v] for v in vids], dtype=np.int32), torch.int32, self.device)

    _hip_ops = None

    def _ops(self):
        if self.ops is not None:
            return self.ops
        if DeviceCiderD._hip_ops is None:
            from .hip import HipOps
            DeviceCiderD._hip_ops = HipOps()
        return DeviceCiderD._hip_ops

    def scores_device(self, ids, clip_idx, end_id=None):
        """CIDEr-D of the id rows ids (int64 (R, L), L <= 64, any row stride) against the references of clips clip_idx (int32 (R,),
        from `index`) -> float64 (R,) tensor on ids' device.  The words of a row are those before its first end_id (default the
        vocabulary's <end>), all L without one.  One launch, no host synchronisation (capturable)."""
        import torch
        out = torch.empty(ids.shape[0], dtype=torch.float64, device=ids.device)
        self._ops().cider_d(ids, clip_idx, self.end_id if end_id is None else int(end_id), self, out)
        return out

    def consensus_device(self, ids, scores=None, temperature=1.0, return_utility=False, end_id=None):
        """Consensus (minimum Bayes risk) ranking of candidate captions against each other -- no references: ids int64 (B, n, L),
        n <= 32 candidates per clip, L <= 64 (rows as in `scores_device`; a view of a wider buffer will do) -> (order (B, n)
        int64, expected (B, n) float64[, util (B, n, n) float64]) on ids' device, what `CiderD.consensus` gives per clip for the
        decoded strings (to rounding, 1e-12), an id outside [0, len(vocab)) being one out-of-vocabulary word that matches
        itself.  scores: float32 (B, n) log-scores for posterior weights exp((s - max) / temperature), None: uniform; a -inf or
        NaN score marks a candidate invalid (expected -inf, ranked last).  One launch (`dlsg_cider_consensus`), no host
        synchronisation (capturable)."""
        import torch
        if ids.dim() != 3:
            raise ValueError('consensus_device ranks ids of shape (B, n, L), not %s' % (tuple(ids.shape),))
        B, n, L = ids.shape
        if not 1 <= n <= MAX_CANDIDATES:
            raise ValueError('consensus_device ranks 1 to %d candidates per clip, not %d' % (MAX_CANDIDATES, n))
        if not 1 <= L <= MAX_CANDIDATE_WORDS:
            raise ValueError('consensus_device reads 1 to %d words per candidate, not %d' % (MAX_CANDIDATE_WORDS, L))
        if not temperature > 0.0:
            raise ValueError('consensus temperature %r must be positive' % (temperature,))
        if scores is not None and (scores.dtype != torch.float32 or tuple(scores.shape) != (B, n)):
            raise ValueError('consensus scores must be float32 of shape %s, not %s %s' % ((B, n), scores.dtype, tuple(scores.shape)))
        dev = ids.device
        order = torch.empty(B, n, dtype=torch.int64, device=dev)
        expected = torch.empty(B, n, dtype=torch.float64, device=dev)
        util = torch.empty(B, n, n, dtype=torch.float64, device=dev) if return_utility else None
        if scores is not None:
            scores = scores.contiguous()
        self._ops().cider_consensus(ids, self.end_id if end_id is None else int(end_id), self, scores, float(temperature), util,
                                    expected, order)
        return (order, expected, util) if return_utility else (order, expected)


# ------------------------------------------------------------------------------------------------ BLEU / ROUGE_L on the device
REF_OOV = 0xFFFF                # a reference word outside the vocabulary in `ref_words`: no id reaches it (V <= 65535)
METRIC_NAMES = ('bleu1', 'bleu2', 'bleu3', 'bleu4', 'rouge_l')
WEIGHT_KEYS = ('cider',) + METRIC_NAMES


def _check_refs(refs):
    for v in refs:
        for r in refs[v]:
            if not r.split():
                raise ValueError('clip %r has a reference with no words' % (v,))


def _host_metrics(refs, vids, hyps):
    """(R, 5) float64: the per-id BLEU-1..4 of `bleu` and ROUGE_L of `rouge_l` for hyps[i] against refs[vids[i]]"""
    memo = {}
    out = np.empty((len(hyps), 5), dtype=np.float64)
    for i, (v, h) in enumerate(zip(vids, hyps)):
        key = (v, h)
        if key not in memo:
            gts, res = {0: refs[v]}, {0: [h]}
            memo[key] = [p[0] for p in bleu(gts, res, 4)[1]] + [rouge_l(gts, res)[1][0]]
        out[i] = memo[key]
    return out


class DeviceCaptionMetrics(object):
    """Sentence-level BLEU-1..4 and ROUGE_L of captions given as vocabulary ids, scored on the GPU (`dlsg_caption_metrics`), and
    the corpus figures of a batch of them (`dlsg_caption_corpus`).  `refs` {vid: [tokenized caption, ...]} as for `CiderD`.  Built
    once and copied to HBM:
      * `clip_off` -- clip c (clips in sorted vid order, the order of `DeviceCiderD`: one `index()` serves both) owns references
        [clip_off[c], clip_off[c + 1]);
      * `ref_off`, `ref_words` -- reference q owns the words ref_words[ref_off[q] : ref_off[q + 1]], mapped through
        `vocab.word2idx` (no `<unk>` mapping); a word outside the vocabulary is REF_OOV, which nothing matches, a sampled
        `<unk>` included.  16 bits a word (stored as int16 bit patterns), hence V <= 65535.
    `scores_device` gives, to rounding (1e-12), what `scores` -- `bleu`'s and `rouge_l`'s per-id values -- gives for the decoded
    strings (decode_tokens: the words before the first <end>); an id outside [0, len(vocab)) is a word that matches nothing.
    The corpus figures of `corpus_device` are `bleu`, `rouge_l` (and the mean of `base`, e.g. CIDEr-D) over the decode_tokens
    strings and these tokenized references.  `scoring.evaluate` is not built on it: `CaptionScorer` re-tokenizes the hypothesis
    STRING, which splits a `<unk>` into three tokens, so its figures differ wherever the model emits `<unk>`.
    `ops`: the kernel binding (None: a `hip.HipOps` made on first use)."""

    def __init__(self, refs, vocab, device='cuda'):
        import torch
        V = len(vocab)
        if V > REF_OOV:
            raise ValueError('DeviceCaptionMetrics keeps 16 bits per word: a vocabulary of %d words is over the %d limit' % (V, REF_OOV))
        _check_refs(refs)
        self.refs, self.vocab, self.device, self.V = refs, vocab, torch.device(device), V
        self.end_id = vocab('<end>')
        self.ops = None
        self.vids = sorted(refs)
        self.vid_index = {v: i for i, v in enumerate(self.vids)}
        w2i = vocab.word2idx
        clip_off, ref_off, words = [0], [0], []
        for v in self.vids:
            for r in refs[v]:
                words.extend(w2i.get(w, REF_OOV) for w in r.split())
                ref_off.append(len(words))
            clip_off.append(len(ref_off) - 1)

        def dev(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.device)
        self.clip_off = dev(np.array(clip_off, dtype=np.int64), torch.int64)
        self.ref_off = dev(np.array(ref_off, dtype=np.int64), torch.int64)
        self.ref_words = dev(np.array(words, dtype=np.uint16).view(np.int16), torch.int16)     # uint16 bits
        self.n_clips = len(self.vids)

    index = DeviceCiderD.index
    _ops = DeviceCiderD._ops

    def scores(self, vids, hyps):
        """host: (R, 5) float64 BLEU-1..4, ROUGE_L of tokenized strings (`bleu`, `rouge_l`)"""
        return _host_metrics(self.refs, vids, hyps)

    def _launch(self, ids, clip_idx, end_id, **out):
        self._ops().caption_metrics(ids, clip_idx, self.end_id if end_id is None else int(end_id), self, **out)

    def scores_device(self, ids, clip_idx, end_id=None):
        """BLEU-1..4 and ROUGE_L of the id rows ids (int64 (R, L), L <= 64, any row stride) against the references of clips
        clip_idx (int32 (R,), from `index`) -> float64 (R, 5) on ids' device.  One launch, no host synchronisation."""
        import torch
        out = torch.empty(ids.shape[0], 5, dtype=torch.float64, device=ids.device)
        self._launch(ids, clip_idx, end_id, scores=out)
        return out

    def stats_device(self, ids, clip_idx, end_id=None):
        """int32 (R, 10): correct[4], guess[4], hypothesis length, closest reference length -- what corpus BLEU sums"""
        import torch
        out = torch.empty(ids.shape[0], 10, dtype=torch.int32, device=ids.device)
        self._launch(ids, clip_idx, end_id, stats=out)
        return out

    def corpus_device(self, ids, clip_idx, base=None, end_id=None):
        """float64 (6,) on the device: corpus Bleu_1..4 and the mean ROUGE_L of the R >= 1 rows, and the mean of `base` (float64
        (R,), e.g. the rows' CIDEr-D; NaN without it).  Two launches, no host synchronisation."""
        import torch
        R = ids.shape[0]
        scores = torch.empty(R, 5, dtype=torch.float64, device=ids.device)
        stats = torch.empty(R, 10, dtype=torch.int32, device=ids.device)
        out = torch.empty(6, dtype=torch.float64, device=ids.device)
        self._launch(ids, clip_idx, end_id, scores=scores, stats=stats)
        self._ops().caption_corpus(stats, scores, base, out)
        return out


def _mix_weights(weights):
    unknown = sorted(set(weights) - set(WEIGHT_KEYS))
    if unknown:
        raise ValueError('reward weights: unknown keys %s (%s)' % (unknown, ', '.join(WEIGHT_KEYS)))
    w = [float(weights.get(k, 0.0)) for k in WEIGHT_KEYS]
    if not any(x != 0.0 for x in w):
        raise ValueError('reward weights: every weight is zero')
    return w


def _mix(w, cider_scores, metrics):
    """w[0] cider + w[1..4] BLEU-1..4 + w[5] ROUGE_L, added in that order, a term with weight 0 left out (the kernel's order)"""
    acc = np.zeros(len(cider_scores) if metrics is None else len(metrics), dtype=np.float64)
    if w[0] != 0.0:
        acc = acc + w[0] * np.asarray(cider_scores, dtype=np.float64)
    for j in range(5):
        if w[j + 1] != 0.0:
            acc = acc + w[j + 1] * metrics[:, j]
    return acc


class MixedReward(object):
    """A weighted sum of CIDEr-D, BLEU-1..4 and ROUGE_L as the self-critical reward (the cider_reward_weight /
    bleu_reward_weight recipe of the usual captioning toolkits), on the host: `scores(vids, hyps)` like `CiderD.scores`.
    `weights`: a dict over 'cider', 'bleu1'..'bleu4', 'rouge_l'; a missing key is 0.  Mind the scales: CIDEr-D is on a x10 scale
    (a good caption scores several units), BLEU and ROUGE_L lie in [0, 1] -- {'cider': 1, 'bleu4': 1} is all but CIDEr-D alone.
    A metric with weight 0 is neither tabulated nor computed."""

    def __init__(self, refs, weights, n=4, sigma=6.0):
        self.w = _mix_weights(weights)
        self.weights = dict(zip(WEIGHT_KEYS, self.w))
        _check_refs(refs)
        self.refs = refs
        self.cider = CiderD(refs, n, sigma) if self.w[0] != 0.0 else None

    def scores(self, vids, hyps):
        c = self.cider.scores(vids, hyps) if self.cider is not None else None
        m = _host_metrics(self.refs, vids, hyps) if any(x != 0.0 for x in self.w[1:]) else None
        return _mix(self.w, c, m)

    def to_device(self, vocab, device='cuda'):
        """the same reward with device tables over `vocab`'s ids (`DeviceMixedReward`); the corpus statistics are not recomputed"""
        return DeviceMixedReward(None, vocab, None, device, _host=self)


class DeviceMixedReward(object):
    """`MixedReward` scored on the GPU for `SCSTTrainer`: `index(vids)` and `scores_device(ids, clip_idx, end_id)` -> float64
    (R,), which is `dlsg_cider_d` followed by `dlsg_caption_metrics` with the CIDEr-D scores as its `base` -- two launches, no
    ATen kernel between them, no host synchronisation.  It owns a `DeviceCiderD` (`cider`; None when the 'cider' weight is 0) and
    a `DeviceCaptionMetrics` (`metrics`; None when only 'cider' is weighted: the CIDEr launch is then the only one, its scores
    scaled in place when the weight is not 1).
    `scores(vids, hyps)` is the host `MixedReward`'s.  Scales: CIDEr-D x10, BLEU and ROUGE_L in [0, 1] (see `MixedReward`)."""

    def __init__(self, refs, vocab, weights, device='cuda', _host=None):
        host = _host if _host is not None else MixedReward(refs, weights)
        self.host, self.w, self.weights, self.vocab = host, host.w, host.weights, vocab
        self.end_id = vocab('<end>')
        self.cider = host.cider.to_device(vocab, device) if host.cider is not None else None
        self.metrics = DeviceCaptionMetrics(host.refs, vocab, device) if any(x != 0.0 for x in self.w[1:]) else None
        self.ops = None

    @property
    def ops(self):
        return self._ops_

    @ops.setter
    def ops(self, ops):
        self._ops_ = ops
        for part in (self.cider, self.metrics):
            if part is not None:
                part.ops = ops

    def scores(self, vids, hyps):
        """MixedReward.scores: tokenized strings on the host"""
        return self.host.scores(vids, hyps)

    def index(self, vids):
        """clip indices of `vids` for `scores_device` (the two tables list the clips in the same order)"""
        return (self.metrics if self.metrics is not None else self.cider).index(vids)

    def scores_device(self, ids, clip_idx, end_id=None):
        """the mixed reward of the id rows ids (int64 (R, L), L <= 64) against the references of clips clip_idx -> float64 (R,)"""
        import torch
        w = self.w
        end_id = self.end_id if end_id is None else int(end_id)
        base = self.cider.scores_device(ids, clip_idx, end_id) if self.cider is not None else None
        if self.metrics is None:
            return base if w[0] == 1.0 else base.mul_(w[0])
        out = torch.empty(ids.shape[0], dtype=torch.float64, device=ids.device)
        self.metrics._ops().caption_metrics(ids, clip_idx, end_id, self.metrics, reward=out, weights=w, base=base)
        return out


# ------------------------------------------------------------------------------------------------ driver (evaluate.py)
class CaptionScorer(object):
    """COCOScorer.score without the Java parts (caption-eval/cocoeval.py:52-103): GT / RES as built by
    convert_data_to_coco_scorer_format / convert_prediction.  Returns ({'Bleu_1'..'Bleu_4','ROUGE_L','CIDEr'}, None)."""

    def score(self, GT, RES, IDs):
        gts = {i: [tokenize(c['caption']) for c in GT[i]] for i in IDs}
        res = {i: [tokenize(c['caption']) for c in RES[i]] for i in IDs}
        out = {}
        b, _ = bleu(gts, res, 4)
        for k in range(4):
            out['Bleu_%d' % (k + 1)] = b[k]
        out['ROUGE_L'] = rouge_l(gts, res)[0]
        out['CIDEr'] = cider(gts, res)[0]
        self.eval = out
        return out, None


def convert_data_to_coco_scorer_format(reference):
    """evaluate.py:16-39: `vid<TAB>sentence` lines -> {vid: [{'video_id', 'cap_id', 'caption'}]}, non-ASCII characters dropped"""
    ref = {}
    with open(reference, 'r') as f:
        for line in f:
            parts = line.split('\t')
            vid, sent = parts[0], parts[1].strip().encode('ascii', 'ignore').decode('ascii')
            ref.setdefault(vid, [])
            ref[vid].append({u'video_id': vid, u'cap_id': len(ref[vid]), u'caption': sent})
    return ref


def convert_prediction(prediction):
    """evaluate.py:50-54"""
    return {str(k): [{u'video_id': str(k), u'caption': v}] for k, v in prediction.items()}


def gather_results(net, eval_loader, decode=None):
    """evaluate.py:62-78 / 101-117: greedy or beam inference over the eval loader -> OrderedDict video id -> sentence.
    `decode`: a dict of `beam_search` options (beam_size, length_penalty, no_repeat_ngram, min_len, num_groups,
    diversity_penalty); the captions are then the best beam of that search.  With the key consensus=reward (a `DeviceCiderD`;
    optionally consensus_weights, consensus_temperature) every beam of that search is kept and the caption is the one the
    others agree with most: row 0 of `consensus.consensus_search`.  With the key constraints=fn, fn(video_ids) -> the batch's
    per-clip constraint lists or packed tensor (`beam.pack_constraints`), the caption is row 0 of
    `constrained_beam_search` with the other options: it contains a word of every constraint (not together with consensus); fn may
    as well return phrases -- lists with strings such as "hot dog", or the tensor of `beam.pack_phrases` --, which that call dispatches.
    With the key rescore=scorer (a model or an `Ensemble`; optionally rescore_mix) every beam of that search is kept and the
    caption is the one the scorer ranks first: row 0 of `rescore.rescore_search` (not together with consensus or constraints).
    With the key exclude=X the search runs under exclusions (`beam.pack_exclusions`): X is an `Exclusions` without a per-clip part,
    which holds for every batch, or fn(video_ids) -> the batch's `Exclusions`; consensus and rescore searches pass it on to their
    beam search, constraints do not take it.
    With the key prefix=X every caption continues a given beginning (`beam.pack_prefix`): X is a (B, P) int64 tensor, which then
    holds for every batch of that size, or fn(video_ids) -> the batch's tensor or per-clip list; every search above passes it on
    to its beam search."""
    import torch
    result = collections.OrderedDict()
    dec = (net.module if hasattr(net, 'module') else net).decoder
    consensus, constraints, rescorer, exclude, prefix = None, None, None, None, None
    if decode is not None and decode.get('prefix') is not None:
        decode = dict(decode)
        prefix = decode.pop('prefix')
        if not callable(prefix) and not torch.is_tensor(prefix):
            raise ValueError('decode: prefix is an int64 tensor (B, P) for every batch, or fn(video_ids) -> prefix')
    if decode is not None and decode.get('exclude') is not None:
        decode = dict(decode)
        exclude = decode.pop('exclude')
        if 'constraints' in decode:
            raise ValueError('decode: exclude and constraints cannot be combined (constrained_beam_search takes no exclusions)')
        if not callable(exclude) and (not isinstance(exclude, tuple) or len(exclude) != 2 or exclude[1] is not None):
            raise ValueError('decode: exclude is an Exclusions without a per-clip part, or fn(video_ids) -> Exclusions')
    if decode is not None and 'rescore' in decode:
        decode = dict(decode)
        rescorer = dict(scorer=decode.pop('rescore'), mix=decode.pop('rescore_mix', 1.0))
        for other in ('consensus', 'constraints'):
            if other in decode:
                raise ValueError('decode: rescore and %s cannot be combined' % other)
    if decode is not None and 'constraints' in decode:
        decode = dict(decode)
        constraints = decode.pop('constraints')
        if 'consensus' in decode:
            raise ValueError('decode: constraints and consensus cannot be combined')
    if decode is not None and 'consensus' in decode:
        decode = dict(decode)
        consensus = dict(reward=decode.pop('consensus'), weights=decode.pop('consensus_weights', 'uniform'),
                         temperature=decode.pop('consensus_temperature', 1.0))
    with torch.no_grad():
        for frames, regions, spatials, video_ids in eval_loader:
            if exclude is not None:
                ex = exclude(video_ids) if callable(exclude) else exclude
                decode['exclude'] = type(ex)(*[None if x is None else x.to(frames.device) for x in ex])
            if prefix is not None:
                px = prefix(video_ids) if callable(prefix) else prefix
                decode['prefix'] = px.to(frames.device) if torch.is_tensor(px) else px
            if decode is None:
                outputs = net(frames, regions, None)[0]
            elif consensus is not None:
                from .consensus import consensus_search
                outputs = consensus_search(net.module if hasattr(net, 'module') else net, frames, regions,
                                           **dict(decode, n_best=1, **consensus))[0][:, 0]
            elif rescorer is not None:
                from .rescore import rescore_search
                outputs = rescore_search(net.module if hasattr(net, 'module') else net, rescorer['scorer'], frames, regions,
                                         n_best=1, mix=rescorer['mix'], **decode)[0][:, 0]
            elif constraints is not None:
                cons = constraints(video_ids)
                if torch.is_tensor(cons):
                    cons = cons.to(frames.device)
                outputs = (net.module if hasattr(net, 'module') else net).constrained_beam_search(
                    frames, regions, cons, **dict(decode, n_best=1))[0][:, 0]
            else:
                outputs = (net.module if hasattr(net, 'module') else net).beam_search(frames, regions, **dict(decode, n_best=1))[0][:, 0]
            ids = outputs.cpu()                                    # host synchronisation: the time-out word is final too
            chk = getattr(getattr(net.module if hasattr(net, 'module') else net, 'ops', None), 'check_persistent', None)
            if chk is not None:
                chk()                                              # a timed-out persistent launch must not pass as captions
            for tokens, vid in zip(ids, video_ids):
                result[vid] = dec.decode_tokens(tokens)
    return result


def merge_rank_results(result, process_group=None):
    """run_gun.py:270-276: every rank decodes its partition of the test clips (`EvalLoader(world_size, rank)`), the per-rank
    caption dicts are exchanged with `all_gather_object` and merged in rank order.  The reference hard-codes four ranks
    (`[None for _ in range(4)]`, `{**r[0], **r[1], **r[2], **r[3]}`); here it is the group's size.  Every rank gets the
    merged dict (the reference scores it on rank 0 only)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(process_group) == 1:
        return result
    parts = [None] * dist.get_world_size(process_group)
    dist.all_gather_object(parts, result, group=process_group)
    merged = collections.OrderedDict()
    for part in parts:
        merged.update(part)
    return merged


def evaluate(net, eval_loader, reference, process_group=None, gather=True, decode=None):
    """evaluate.py:56-98 -> (scores, result).  `reference`: dict from convert_data_to_coco_scorer_format.  Inside an
    initialised process group (several GPUs, each with its own partition of the clips in `eval_loader`) the ranks' results are
    merged first (`evaluate_multi_gpu` of evaluate.py:120-134 on the gathered dict, run_gun.py:268-281), so the scores cover
    the whole test set on every rank; gather=False scores this rank's partition only.  `decode`: see gather_results."""
    result = gather_results(net, eval_loader, decode)
    if gather:
        result = merge_rank_results(result, process_group)
    pred = convert_prediction(result)
    scores, _ = CaptionScorer().score(reference, pred, list(pred.keys()))
    return scores, result


def perplexity(scorer, loader):
    """Held-out likelihood of the reference captions a `data.TrainLoader` yields (captions_per_clip = n included: the encoder then
    runs once per clip) under `scorer`, a model or an `Ensemble`: the cheap validation signal between two full evaluations.
    Returns dict(nll, ppl, words, top1, top5): the mean negative log-probability per counted word, its exponential, the number of
    counted words, and the fraction of them the scorer ranks first / among its five best, teacher-forced.  The counted positions
    are those `dlsg_ce_ragged` counts for the same batch in the train step: t < min(cap_len, L).  Per batch one teacher-forced
    pass per member without dropout and one `seq_logprob` launch; the sums are kept on the device in float64 and read once at
    the end."""
    import torch
    from .hip import host_to_device
    from .ensemble import MODES
    from .rescore import as_ensemble
    ens = as_ensemble(scorer)
    acc = None
    with torch.no_grad():
        for frames, regions, _, captions, _, cap_lens, _ in loader:
            lens = cap_lens if torch.is_tensor(cap_lens) else host_to_device(list(cap_lens), torch.int64, captions.device)
            logits = ens.teacher_logits(frames, regions, captions, seq_per_clip=captions.shape[0] // frames.shape[0])
            _, counted, lp, _, rank = ens.ops.seq_logprob(logits, ens.weights, MODES[ens.mode], captions.contiguous(), lens.contiguous(),
                                                          want_ranks=True)
            live = rank >= 0
            part = torch.stack([-lp.double().sum(), counted.sum().double(), (rank == 0).sum().double(),
                                (live & (rank < 5)).sum().double()])
            acc = part if acc is None else acc + part
    if acc is None:
        raise ValueError('perplexity: the loader yielded no batch')
    nll, words, top1, top5 = acc.tolist()                              # the one host read
    chk = getattr(ens.ops, 'check_persistent', None)
    if chk is not None:
        chk()
    if words == 0:
        raise ValueError('perplexity: no counted word')
    return dict(nll=nll / words, ppl=math.exp(nll / words), words=int(words), top1=top1 / words, top5=top5 / words)

"""The module the reference's decoder imports and never shipped (`from LanguageModel.Ngram import Ngram`, Decoder.py:17): word
n-gram counts, and their flat form for the decoder on the device.

What the reference shows of it: `main` builds `Ngram(n=i + 1).init_gram()` for i < n (Decoder.py:200-204), and
`passing_between_word` asks `ngram.ngram(word)` for a dictionary {following word: count} and turns count / sum into a log score
(:146-156; the function raises on its first arithmetic line and ends in `Token()`).  Everything else here is this project's:
add-one unigrams, Witten-Bell bigrams with ARPA-shaped backoff, and `compile`, which lays the scores out for pcl_lm_upload.

Logarithms are NATURAL (the acoustic scores are): the reference wrote math.log10 (:155); a base is a constant factor on every
language-model term, which `lm_scale` covers (lm_scale = 1 / ln 10 gives its base).  Pure Python / NumPy.
"""
import json
import os

import numpy as np

BOS = '<s>'          # the sentence start: word id 0, spelled by no tree node


class Ngram(object):
    def __init__(self, n=2):
        if n not in (1, 2):
            raise ValueError('Ngram: n = %r (unigrams and bigrams only)' % (n,))
        self.n = n
        self.words = [BOS]                   # id -> string
        self.index = {BOS: 0}
        self.uni_count = np.zeros(1, dtype=np.int64)
        self.bi_count = {}                   # predecessor id -> {successor id: count}

    # ------------------------------------------------------------------ counts
    def count(self, sentences, vocabulary):
        """sentences: lists of words.  Unigram counts run over the in-vocabulary words; bigram counts (n = 2) take the sentence
        start as the first predecessor; a pair with a member outside the vocabulary is not counted."""
        self.words = [BOS] + [w for w in dict.fromkeys(vocabulary) if w != BOS]
        self.index = {w: i for i, w in enumerate(self.words)}
        self.uni_count = np.zeros(len(self.words), dtype=np.int64)
        self.bi_count = {}
        for sentence in sentences:
            prev = 0
            for word in sentence:
                w = self.index.get(word)
                if w is None or w == 0:
                    prev = None
                    continue
                self.uni_count[w] += 1
                if self.n >= 2 and prev is not None:
                    row = self.bi_count.setdefault(prev, {})
                    row[w] = row.get(w, 0) + 1
                prev = w
        return self

    def ngram(self, word):
        """{following word: count}: the call of Decoder.py:151.  With n = 1 every word follows every word: the unigram counts."""
        if self.n == 1:
            return {self.words[w]: int(c) for w, c in enumerate(self.uni_count) if c}
        v = self.index.get(word)
        return {self.words[w]: int(c) for w, c in self.bi_count.get(v, {}).items()}

    def save_gram(self, path='ngram'):
        """The counts as .npy files plus the word list, one directory per order (the model tree's style)."""
        d = os.path.join(path, '%dgram' % self.n)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'words.json'), 'w') as f:
            json.dump(self.words, f, ensure_ascii=False)
        np.save(os.path.join(d, 'unigram.npy'), self.uni_count)
        pairs = [(v, w, c) for v in sorted(self.bi_count) for w, c in sorted(self.bi_count[v].items())]
        np.save(os.path.join(d, 'bigram.npy'), np.array(pairs, dtype=np.int64).reshape(-1, 3))

    def init_gram(self, path='ngram'):
        d = os.path.join(path, '%dgram' % self.n)
        with open(os.path.join(d, 'words.json')) as f:
            self.words = list(json.load(f))
        self.index = {w: i for i, w in enumerate(self.words)}
        self.uni_count = np.load(os.path.join(d, 'unigram.npy')).astype(np.int64)
        self.bi_count = {}
        for v, w, c in np.load(os.path.join(d, 'bigram.npy')).reshape(-1, 3).tolist():
            self.bi_count.setdefault(v, {})[w] = c
        return self

    # ------------------------------------------------------------------ probabilities (natural log)
    def unigram_prob(self):
        """P(w) = (c(w) + 1) / (N + V) over the V = W - 1 real words; the sentence start gets the same formula with c = 0 (it is
        never a successor: no node spells it)."""
        V = len(self.words) - 1
        return (self.uni_count + 1.0) / (float(self.uni_count.sum()) + V)

    def bigram_rows(self):
        """Witten-Bell.  Per predecessor v with successors: (ids ascending, P(w|v) = (c(v,w) + T(v) P(w)) / (c(v.) + T(v)),
        bow(v) = T(v) / (c(v.) + T(v))); T(v) = distinct successors, c(v.) = their total.  Returns ({v: (ids, probs)}, bow[W]);
        bow = 1 where v has no successors (and everywhere with n = 1)."""
        pw = self.unigram_prob()
        bow = np.ones(len(self.words))
        rows = {}
        for v, succ in self.bi_count.items():
            ids = np.array(sorted(succ), dtype=np.int64)
            c = np.array([succ[w] for w in ids.tolist()], dtype=np.float64)
            T, tot = float(len(ids)), float(c.sum())
            rows[v] = (ids, (c + T * pw[ids]) / (tot + T))
            bow[v] = T / (tot + T)
        return rows, bow

    def prob(self, v, w):
        """P(w | v) by ids, backed off: what the compiled tables hold before the logarithm."""
        rows, bow = self.bigram_rows()
        if v in rows:
            ids, p = rows[v]
            k = int(np.searchsorted(ids, w))
            if k < len(ids) and ids[k] == w:
                return float(p[k])
        return float(bow[v] * self.unigram_prob()[w])

    # ------------------------------------------------------------------ flat form for the device
    def compile(self, tree, lm_scale=1.0, word_penalty=0.0):
        """The tables pcl_lm_upload takes, for the tree of PronunciationLexicon.compile:
            uni[W] = lm_scale ln P(w) + word_penalty,  bow[W] = lm_scale ln bow(v),
            row_ptr[W + 1] (int64) / col (ascending in a row) / val = lm_scale ln P(w|v) + word_penalty,
            node_word_ptr[n_nodes + 1] / node_word_ids: the ids of tree['words'][node] in that order,  words: id -> string.
        The multiply and the add are two NumPy operations (two roundings).  Words of the tree the counts have not seen join the
        vocabulary with count 0."""
        words, index = list(self.words), dict(self.index)
        for ws in tree['words']:
            for w in ws:
                if w not in index:
                    index[w] = len(words)
                    words.append(w)
        full = self
        if len(words) != len(self.words):
            full = Ngram(self.n)
            full.words, full.index = words, index
            full.uni_count = np.concatenate([self.uni_count, np.zeros(len(words) - len(self.words), dtype=np.int64)])
            full.bi_count = self.bi_count
        W = len(words)
        rows, bow = full.bigram_rows()
        scale, pen = np.float64(lm_scale), np.float64(word_penalty)
        uni = scale * np.log(full.unigram_prob())
        uni = uni + pen
        row_ptr = np.zeros(W + 1, dtype=np.int64)
        for v in range(W):
            row_ptr[v + 1] = row_ptr[v] + (len(rows[v][0]) if v in rows else 0)
        col = np.concatenate([rows[v][0] for v in sorted(rows)] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
        val = scale * np.log(np.concatenate([rows[v][1] for v in sorted(rows)] + [np.zeros(0)]))
        val = val + pen
        nptr = np.zeros(len(tree['words']) + 1, dtype=np.int32)
        ids = []
        for i, ws in enumerate(tree['words']):
            ids.extend(index[w] for w in ws)
            nptr[i + 1] = len(ids)
        return dict(W=W, uni=uni, bow=scale * np.log(bow), row_ptr=row_ptr, col=col, val=val, node_word_ptr=nptr,
                    node_word_ids=np.array(ids, dtype=np.int32), words=words)


def lm_score(lm, v, w):
    """lm(v, w) of the compiled tables: the explicit entry, else bow[v] + uni[w] -- the rule the device applies, on the host (the
    decoder uses it to pick the word still pending at a final token's node)."""
    lo, hi = int(lm['row_ptr'][v]), int(lm['row_ptr'][v + 1])
    k = lo + int(np.searchsorted(lm['col'][lo:hi], w))
    if k < hi and lm['col'][k] == w:
        return lm['val'][k]
    return lm['bow'][v] + lm['uni'][w]


def best_word(lm, v, node):
    """(chosen word id, its score): max over the node's homophones of lm(v, w), the first on ties."""
    best, word = None, -1
    for w in lm['node_word_ids'][lm['node_word_ptr'][node]:lm['node_word_ptr'][node + 1]].tolist():
        x = lm_score(lm, v, w)
        if best is None or x > best:
            best, word = x, w
    return word, best

"""Reference and checker of the Hamming tests (numpy only; nothing here touches the GPU or the library).

The score of a (row, query) pair is the exact integer popcount(row ^ query); the tie rule leaves free which of several equal
scores sit at the k-th place and in what order equal scores come — and nothing else.  check_hamming_lists checks exactly that.
"""
import numpy as np


def hamming_reference(base_words, query_words, chunk=1024):
    """int64 [nq][n]: popcount of XOR through np.unpackbits on the uint8 view, `chunk` base rows at a time"""
    b = np.ascontiguousarray(base_words)
    q = np.ascontiguousarray(query_words)
    b8 = b.view(np.uint8).reshape(b.shape[0], -1)
    q8 = q.view(np.uint8).reshape(q.shape[0], -1)
    assert b8.shape[1] == q8.shape[1]
    out = np.zeros((q8.shape[0], b8.shape[0]), np.int64)
    for o in range(0, b8.shape[0], chunk):
        x = b8[None, o:o + chunk, :] ^ q8[:, None, :]
        out[:, o:o + chunk] = np.unpackbits(x, axis=2).sum(axis=2, dtype=np.int64)
    return out


def check_hamming_lists(keys, scores, counts, ref, k, threshold=None, admissible=None, key_of_row=None, what=""):
    """keys / scores [nq][k], counts [nq] against ref [nq][n] (hamming_reference).  admissible: bool [n] (or [nq][n]) — rows a
    search may return (not excluded, not a hole); key_of_row: uint64 [n], default the row number.  Raises AssertionError."""
    nq, n = ref.shape
    key_of_row = np.arange(n, dtype=np.uint64) if key_of_row is None else np.asarray(key_of_row, np.uint64)
    row_of_key = {int(key): i for i, key in enumerate(key_of_row)}
    adm = np.ones((nq, n), bool) if admissible is None else np.broadcast_to(np.asarray(admissible, bool), (nq, n))
    for q in range(nq):
        ok = adm[q].copy()
        if threshold is not None:
            ok &= ref[q] <= threshold
        want = np.sort(ref[q][ok])[:k]
        c = int(counts[q])
        assert c == want.size, "%s query %d: count %d, expected %d" % (what, q, c, want.size)
        got_s = np.asarray(scores[q, :c])
        assert np.array_equal(got_s, want.astype(np.float32)), "%s query %d: scores %r, expected %r" % (what, q, got_s, want)
        got_k = [int(x) for x in keys[q, :c]]
        assert len(set(got_k)) == c, "%s query %d: duplicate keys" % (what, q)
        rows = []
        for j, key in enumerate(got_k):
            assert key in row_of_key, "%s query %d: unknown key %d" % (what, q, key)
            r = row_of_key[key]
            assert ok[r], "%s query %d: key %d is not admissible" % (what, q, key)
            assert float(ref[q, r]) == float(got_s[j]), "%s query %d: key %d scored %r, its distance is %d" % (what, q, key, got_s[j], ref[q, r])
            rows.append(r)
        if c:
            must = np.nonzero(ok & (ref[q] < float(got_s[-1])))[0]
            missing = set(int(r) for r in must) - set(rows)
            assert not missing, "%s query %d: rows %r are strictly better than the last score and missing" % (what, q, sorted(missing)[:5])

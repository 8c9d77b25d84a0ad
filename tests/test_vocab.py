"""String-vocabulary kernels (csrc/vocab.hip) vs the exact host implementation of
tft.compute_and_apply_vocabulary semantics in mifx.transform.api."""
import collections
import functools

import numpy as np
import pytest

from mifx.ops import vocab as V
from mifx.transform import api as tft


def _column(n=50000, seed=0):
    rng = np.random.default_rng(seed)
    # Zipf-ish company names + payment types + empties/None/bytes/unicode (taxi-like string columns)
    base = [f"company_{i}" for i in range(3000)] + ["Cash", "Credit Card", "No Charge", "", "Dispute", "Ünïcødé"]
    p = 1.0 / np.arange(1, len(base) + 1) ** 1.1
    idx = rng.choice(len(base), size=n, p=p / p.sum())
    col = [base[i] for i in idx]
    col[::97] = [None] * len(col[::97])
    col[5::211] = [b"Cash"] * len(col[5::211])
    return col


def test_pack_strings_roundtrip():
    col = ["a", "", None, b"xyz", "Ünï"]
    buf, offs, get = V.pack_strings(col)
    assert offs.tolist()[0] == 0 and offs[-1] == len("axyzÜnï".encode())
    got = [bytes(buf[offs[i]:offs[i + 1]]).decode() for i in range(len(col))]
    assert got == ["a", "", "", "xyz", "Ünï"] == [get(i) for i in range(len(col))]


def test_pack_strings_arrow_zero_copy_matches_list():
    import pyarrow as pa

    col = ["a", None, "", "xyz", "Ünï"] * 3
    arr = pa.chunked_array([pa.array(col[:7]), pa.array(col[7:])])
    buf, offs, get = V.pack_strings(arr)
    got = [bytes(buf[offs[i]:offs[i + 1]]).decode() for i in range(len(col))]
    assert got == [c or "" for c in col] == [get(i) for i in range(len(col))]
    sl = pa.array(col).slice(3, 5)  # non-zero Arrow offset
    buf, offs, get = V.pack_strings(sl)
    assert [bytes(buf[offs[i]:offs[i + 1]]).decode() for i in range(5)] == [c or "" for c in col[3:8]]
    assert V.vocabulary(arr, device=None) == V.vocabulary(col, device=None)


def test_fnv_matches_transform_fingerprint():
    for s in ["", "a", "Credit Card", "Ünïcødé", "x" * 300]:
        assert V.fnv1a64(s.encode()) == tft.fingerprint64(s)


def test_host_vocabulary_matches_transform_api():
    col = _column(5000)
    with tft._phase("analyze", tft.TransformState()):
        ref = tft.vocabulary(col, top_k=1000)
    assert V.vocabulary(col, top_k=1000) == ref
    got = V.apply_vocabulary(col, ref, default_value=-1, num_oov_buckets=10)
    assert np.array_equal(got, tft.apply_vocabulary(col, ref, default_value=-1, num_oov_buckets=10))


def test_order_ties_by_token_descending():
    assert V.order_vocabulary(["a", "b", "c"], [2, 2, 5]) == ["c", "b", "a"]
    assert V.order_vocabulary(["a", "b", "c"], [2, 2, 5], top_k=2) == ["c", "b"]
    assert V.order_vocabulary(["a", "b", "c"], [1, 2, 5], frequency_threshold=2) == ["c", "b"]


@pytest.mark.gpu
def test_gpu_hash_matches_host():
    col = _column(20000, seed=1)
    got = V.hash_strings(col, device="cuda")
    ref = V.hash_strings(col, device=None)
    assert got.dtype == np.uint64 and np.array_equal(got, ref)


@pytest.mark.gpu
def test_gpu_count_and_vocabulary_match_host():
    col = _column(200000, seed=2)
    toks, counts = V.count_unique(col, device="cuda")
    ht, hc = V.count_unique(col, device=None)
    assert dict(zip(toks, counts)) == dict(zip(ht, hc))
    for top_k, thr in ((None, None), (1000, None), (50, 3)):
        assert V.vocabulary(col, top_k, thr, device="cuda") == V.vocabulary(col, top_k, thr, device=None)


@pytest.mark.gpu
@pytest.mark.parametrize("oov,default", [(10, -1), (0, -1), (0, 7)])
def test_gpu_apply_vocabulary_matches_host(oov, default):
    col = _column(100000, seed=3)
    vocab = V.vocabulary(col[:20000], top_k=1000)
    got = V.apply_vocabulary(col, vocab, default_value=default, num_oov_buckets=oov, device="cuda")
    ref = tft.apply_vocabulary(col, vocab, default_value=default, num_oov_buckets=oov)
    assert np.array_equal(got, ref)


@pytest.mark.gpu
def test_transform_api_uses_gpu_vocab_path(monkeypatch):
    """compute_and_apply_vocabulary inside analyze(device='cuda') routes through the HIP kernels
    and yields exactly the CPU result."""
    calls = []
    real = V.count_unique
    monkeypatch.setattr(V, "count_unique", lambda *a, **k: calls.append(k.get("device")) or real(*a, **k))
    col = np.array(_column(60000, seed=4), dtype=object)

    def fn(inputs):
        return {"c": tft.compute_and_apply_vocabulary(inputs["c"], top_k=1000, num_oov_buckets=10)}

    out_gpu, st_gpu = tft.analyze(fn, {"c": col}, device="cuda")
    out_cpu, st_cpu = tft.analyze(fn, {"c": col}, device=None)
    assert any(d is not None for d in calls)
    assert st_gpu.entries == st_cpu.entries
    assert np.array_equal(out_gpu["c"], out_cpu["c"])


@pytest.mark.gpu
def test_gpu_arrow_column_matches_host():
    import pyarrow as pa

    col = [v.decode() if isinstance(v, bytes) else v for v in _column(100000, seed=5)]
    arr = pa.chunked_array([pa.array(col[:40000]), pa.array(col[40000:])])
    vocab = V.vocabulary(arr, top_k=1000, device="cuda")
    assert vocab == V.vocabulary(col, top_k=1000, device=None)
    got = V.apply_vocabulary(arr, vocab, default_value=-1, num_oov_buckets=10, device="cuda")
    assert np.array_equal(got, tft.apply_vocabulary(col, vocab, default_value=-1, num_oov_buckets=10))


# ------------------------------------------------------------------------- overflow paths and degenerate columns
# Which kernel path a case reaches (csrc/vocab.hip):
#   vocab_count_lds  each block pre-aggregates ~2048 rows in a 2048-slot LDS table with 32 linear probes; a row whose
#                    key finds no slot goes straight to the global table (global_insert with count 1). The grid is
#                    max(256, ceil(n / 2048)) blocks, so below n = 524,288 + 2048 a block sees at most 2048 rows of a
#                    Zipf column and the LDS table never fills. _high_cardinality() is n = 600,000 -> 293 blocks;
#                    195 of them read 2048 rows holding ~1,850 distinct keys, which do not all find a slot
#                    (test_lds_table_model_overflows counts the misses on the CPU), 98 read the 5 hot tokens (and the
#                    column's last 640 rows).
#   vocab_insert     a repeated vocabulary entry -> flag -> DeviceVocabulary.ok False -> host lookup.
#   vocab_lookup     empty table (n_vocab = 0: every probe ends on an empty slot), "" as a vocabulary entry, OOV
#                    buckets 0 / 1 / 10, a default value beyond int32.
N_HIGH, N_DISTINCT, HOT = 600_000, 200_000, ["Cash", "Credit Card", "No Charge", "Dispute", "Unknown"]
GRID_HIGH, DENSE_BLOCKS = 293, 195  # ceil(600,000 / 2048) blocks; block b reads the 256-row chunks c with c % 293 == b


@functools.lru_cache(maxsize=None)
def _high_cardinality():
    """200,000 rows drawn from 5 hot tokens, laid on the rows that blocks 195 .. 292 read (they pre-aggregate 2048
    rows into 5 LDS slots), and 200,000 distinct tokens twice each on all other rows: token i at the i-th of those
    rows and again 300,000 or 100,000 of them later, so far apart and mostly in another block. Blocks 0 .. 194 thus
    see 2048 rows with about 1,850 distinct keys against 2048 LDS slots and 32 probes: dozens of rows per block
    must take the direct global insert, while the other occurrence of the same key may sit in an LDS table."""
    rng = np.random.default_rng(7)
    rows = np.arange(N_HIGH)
    hot_rows = np.flatnonzero((rows // 256) % GRID_HIGH >= DENSE_BLOCKS)[:N_HIGH - 2 * N_DISTINCT]
    other = np.setdiff1d(rows, hot_rows)
    toks = np.array([f"t{i}" for i in range(N_DISTINCT)], dtype=object)
    col = np.empty(N_HIGH, dtype=object)
    col[hot_rows] = np.array(HOT, dtype=object)[rng.integers(0, len(HOT), hot_rows.size)]
    col[other[:N_DISTINCT]] = toks
    col[other[N_DISTINCT:]] = np.roll(toks, N_DISTINCT // 2)
    col = col.tolist()
    return col, collections.Counter(col)


def _fnv_numpy(col):
    """FNV-1a of every row, vectorised over the packed bytes (uint64 arithmetic wraps like the kernel's)."""
    buf, offs, _ = V.pack_strings(col)
    lens = np.diff(offs)
    h = np.full(len(col), V._FNV_OFF, dtype=np.uint64)
    for j in range(int(lens.max())):
        live = lens > j
        h[live] = (h[live] ^ buf[offs[:-1][live] + j].astype(np.uint64)) * np.uint64(V._FNV_PRIME)
    return h


def _slot0(key: int, mask: int) -> int:
    return ((((key ^ (key >> 29)) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 32) & mask


def test_lds_table_model_overflows():
    """A sequential model of vocab_count_lds' LDS table (2048 slots, 32 probes, the kernel's slot hash) over the
    rows that blocks 0, 100 and 194 (dense) and 250 (hot) of the 293-block grid read from the high-cardinality
    column: each dense block has dozens of rows that find no LDS slot and must take the direct global insert, the
    hot block folds its 2048 rows into 5 slots. (The device inserts in another order; with ~1,850 keys for 2048
    slots the table is about 90% full in any order.)"""
    col, want = _high_cardinality()
    assert len(want) == N_DISTINCT + len(HOT) and sum(want[t] for t in HOT) == N_HIGH - 2 * N_DISTINCT
    assert all(want[f"t{i}"] == 2 for i in (0, 1, 99_999, 100_000, N_DISTINCT - 1))
    assert min(abs(col.index(f"t{i}") - (N_HIGH - 1 - col[::-1].index(f"t{i}"))) for i in (0, 99_999, 100_000)) > 99_999
    with np.errstate(over="ignore"):
        h = _fnv_numpy(col)
    assert [int(h[i]) for i in (0, 123_456, 599_999)] == [V.fnv1a64(col[i].encode()) for i in (0, 123_456, 599_999)]
    assert (N_HIGH + 2047) // 2048 == GRID_HIGH > 256
    for blk in (0, 100, 194, 250):
        rows = np.concatenate([np.arange(s, min(s + 256, N_HIGH)) for s in range(blk * 256, N_HIGH, GRID_HIGH * 256)])
        assert rows.size == 2048
        table, failed = {}, 0
        for i in rows.tolist():
            k = int(h[i])
            s = _slot0(k, 2047)
            for _ in range(32):
                if table.setdefault(s, k) == k:
                    break
                s = (s + 1) & 2047
            else:
                failed += 1
        print(f"block {blk}: {len(table)} LDS slots used, {failed} rows to the global table")
        if blk < DENSE_BLOCKS:
            assert failed > 0 and len(table) >= 1800, (blk, failed, len(table))  # 46, 36 and 27 rows
        else:
            assert failed == 0 and len(table) == len(HOT), (blk, failed, len(table))


def test_fnv_known_vectors():
    """Published FNV-1a 64-bit test vectors pin the host hash the device hash is compared with."""
    assert V.fnv1a64(b"") == 0xCBF29CE484222325
    assert V.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    assert V.fnv1a64(b"foobar") == 0x85944171F73967E8
    assert V.hash_strings(["", None, b"a", "foobar"]).tolist() == [0xCBF29CE484222325, 0xCBF29CE484222325,
                                                                   0xAF63DC4C8601EC8C, 0x85944171F73967E8]


DEGENERATE = {
    "n1": ["only"],
    "all-empty": ["", None, "", b"", None] * 60,
    "embedded-nul": ["a\x00b", "a\x00", "a", "\x00", "", "a\x00b", b"a\x00b", "\x00\x00"] * 40,
    "10kb-token": ["x" * 10_240, "x" * 10_239, "y", "x" * 10_240, "y" * 3] * 5,
    "last-byte": ["company_1230", "company_1231", "company_1230", "company_123"] * 70,
    "prefix": ["Credit", "Credit Card", "Credit Card", "Credit ", "C", ""] * 50,
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_host_count_and_lookup_on_degenerate_columns(name):
    """The host results the device is compared with, against collections.Counter and a plain dict lookup."""
    col = DEGENERATE[name]
    strs = ["" if v is None else (v.decode() if isinstance(v, bytes) else v) for v in col]
    toks, counts = V.count_unique(col, device=None)
    assert dict(zip(toks, counts)) == collections.Counter(strs) and len(set(toks)) == len(toks)
    vocab = V.vocabulary(col)
    assert sorted(vocab) == sorted(set(strs))
    got = V.apply_vocabulary(col, vocab[:1], default_value=2**40, num_oov_buckets=0)
    assert got.dtype == np.int64 and got.tolist() == [0 if s == vocab[0] else 2**40 for s in strs]
    got = V.apply_vocabulary(col, [], default_value=-1, num_oov_buckets=10)
    assert got.tolist() == [V.fnv1a64(s.encode()) % 10 for s in strs]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_gpu_degenerate_columns_match_host(name):
    """One row; only empty strings; embedded NUL bytes (lengths come from the offsets, not a terminator); a 10 KB
    token and its 10,239-byte prefix; tokens differing in the last byte; a token that is a prefix of another: hashes,
    counts, vocabulary and lookup all equal the host's."""
    col = DEGENERATE[name]
    assert np.array_equal(V.hash_strings(col, device="cuda"), V.hash_strings(col, device=None))
    got = V.count_unique(col, device="cuda")
    assert got is not None
    ht, hc = V.count_unique(col, device=None)
    assert dict(zip(*got)) == dict(zip(ht, hc)) and len(got[0]) == len(ht)
    vocab = V.vocabulary(col, device="cuda")
    assert vocab == V.vocabulary(col, device=None)
    for keep in (vocab, vocab[:1]):
        for oov in (0, 10):
            dev = V.apply_vocabulary(col, keep, default_value=-1, num_oov_buckets=oov, device="cuda")
            assert np.array_equal(dev, V.apply_vocabulary(col, keep, default_value=-1, num_oov_buckets=oov))


@pytest.mark.gpu
def test_gpu_high_cardinality_count_overflows_lds_tables():
    """vocab_count_lds' probe-overflow path (header comment above): 200,000 keys counted twice each, in different
    blocks and -- for many -- once through an LDS table and once by the direct global insert, next to 5 hot keys
    that every block pre-aggregates. The device must finish the column itself (not None: no overflow or collision
    flag), equal collections.Counter of the host strings, and give the same result on a second run."""
    col, want = _high_cardinality()
    got = V.count_unique(col, device="cuda")
    assert got is not None
    toks, counts = got
    assert len(toks) == len(want) == N_DISTINCT + len(HOT)
    assert dict(zip(toks, counts)) == want
    again = V.count_unique(col, device="cuda")
    assert again is not None and dict(zip(*again)) == want
    assert sorted(zip(*again)) == sorted(zip(toks, counts))


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [None, 1000])
def test_gpu_high_cardinality_vocabulary_order(top_k):
    """The tft ordering over the overflowing column: 5 hot tokens, then 200,000 tokens tied at 2 by token
    descending, cut at top_k."""
    col, want = _high_cardinality()
    ref = V.order_vocabulary(list(want), list(want.values()), top_k)
    assert V.vocabulary(col, top_k, device="cuda") == ref
    assert len(ref) == (top_k or N_DISTINCT + len(HOT)) and set(ref[:5]) == set(HOT)


@pytest.mark.gpu
@pytest.mark.parametrize("default", [-1, 2**40])
@pytest.mark.parametrize("oov", [0, 1, 10])
@pytest.mark.parametrize("vocab", [[], [""], ["Cash", "", "Credit Card"]],
                         ids=["empty", "only-empty-string", "with-empty-string"])
def test_gpu_apply_vocabulary_edge_vocabularies(vocab, oov, default):
    """vocab_lookup with an empty vocabulary (everything OOV-bucketed or the default), "" as an entry (missing
    values map to its id), 0 / 1 / 10 OOV buckets and a default value beyond int32, which comes back as int64."""
    col = _column(3000, seed=6)
    dv = V.DeviceVocabulary(vocab, "cuda")
    assert dv.ok
    got = dv.lookup(col, default_value=default, num_oov_buckets=oov)
    assert got.dtype == np.int64
    assert np.array_equal(got, V._lookup_host(col, vocab, default, oov))
    assert np.array_equal(got, V.apply_vocabulary(col, vocab, default, oov, device="cuda"))
    if not oov:
        assert (got == default).any()
    if "" in vocab:
        assert (got[::97] == vocab.index("")).all()  # the None rows


@pytest.mark.gpu
def test_gpu_duplicate_vocabulary_entry_uses_host_lookup():
    """A repeated entry makes vocab_insert meet its own key: the flag is raised, DeviceVocabulary.ok is False and
    lookup() is the host's (first-wins would differ from the dict's last-wins index)."""
    col = _column(3000, seed=7)
    vocab = ["Cash", "Credit Card", "Cash", "company_0"]
    dv = V.DeviceVocabulary(vocab, "cuda")
    assert not dv.ok
    for oov, default in ((0, -1), (10, -1), (0, 2**40)):
        got = dv.lookup(col, default_value=default, num_oov_buckets=oov)
        assert got.dtype == np.int64 and np.array_equal(got, V._lookup_host(col, vocab, default, oov))
    assert 2 in got and 0 not in got  # "Cash" -> its last index

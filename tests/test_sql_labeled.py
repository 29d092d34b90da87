"""vector_full_scan_labeled / vector_quantize_scan_labeled(table, column, vector, k, label_column, label) -> (id, distance) and the batch
forms (..., queries, k, label_column, labels) -> (query, id, distance): the labeled scans of the C-ABI behind SQL.  The yardstick is the
statement they replace: the stream function's rows JOINed to the table WHERE t.label = ? ORDER BY distance, id LIMIT k."""
import os
import sqlite3
import struct

import numpy as np
import pytest

import datagen as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_OPT = {dg.F32: "FLOAT32", dg.U8: "UINT8"}
DIST_OPT = {dg.L2: "L2", dg.COSINE: "COSINE"}
PAIRS = (("vector_full_scan_labeled", "vector_full_scan_batch_labeled", "vector_full_scan_stream"),
         ("vector_quantize_scan_labeled", "vector_quantize_scan_batch_labeled", "vector_quantize_scan_stream"))
N, DIM = 3001, 48


@pytest.fixture(scope="module")
def ext_path():
    import __graft_entry__ as g
    b = g._load_build()
    b.build_gpu_library()
    p = b.build_extension()
    assert p and os.path.exists(p)
    return p[:-3]


def connect(path, file=":memory:"):
    db = sqlite3.connect(file, isolation_level=None, check_same_thread=False, timeout=60)
    db.enable_load_extension(True)
    db.load_extension(path)
    return db


def label_of(j):
    """row j + 1: tenants 0..6 in runs of 50 rows, every 11th row NULL, every 13th a text"""
    if (j + 1) % 11 == 0:
        return None
    if (j + 1) % 13 == 0:
        return "seven"
    return (j // 50) % 7


def load_table(db, rows, vt, metric, extra=""):
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, label, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, label, v) VALUES (?, ?, ?)", [(j + 1, label_of(j), rows[j].tobytes()) for j in range(rows.shape[0])])
    db.execute("COMMIT")
    db.execute("SELECT vector_init('t', 'v', ?)", ("type=%s,dimension=%d,distance=%s%s" % (TYPE_OPT[vt], rows.shape[1], DIST_OPT[metric], extra),))


def bits(rows):
    return [tuple(r[:-1]) + (struct.pack("<d", r[-1]),) for r in rows]


def want(db, stream, q, label, k):
    return db.execute("SELECT s.id, s.distance FROM %s('t','v',?) AS s JOIN t ON t.id = s.id WHERE t.label = ? AND typeof(t.label) = 'integer' "
                      "AND s.distance < 9e999 ORDER BY s.distance, s.id LIMIT ?" % stream, (q, label, k)).fetchall()


def single(db, fn, q, k, label):
    return db.execute("SELECT id, distance FROM %s('t','v',?,?,'label',?)" % fn, (q, k, label)).fetchall()


def check(db, fns, q, labels=(0, 3, 6, 99), ks=(1, 20, 64)):
    fn, _, stream = fns
    for label in labels:
        for k in ks:
            w = want(db, stream, q, label, k)
            assert bits(single(db, fn, q, k, label)) == bits(w), (fn, label, k)
            if label == 99:
                assert w == []                                   # a label nobody has: no rows


def check_batch(db, fns, qs, qlabels, k=20):
    """the batch function agrees with the single one per query"""
    fn, bfn, _ = fns
    got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,'label',?)" % bfn,
                     (b"".join(qs), k, struct.pack("<%dq" % len(qlabels), *qlabels))).fetchall()
    exp = []
    for i, (q, label) in enumerate(zip(qs, qlabels)):
        exp += [(i,) + r for r in single(db, fn, q, k, label)]
    assert bits(got) == bits(exp), (bfn, qlabels)
    assert any(r[0] == len(qs) - 1 for r in got)


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert {p[0] for p in PAIRS} | {p[1] for p in PAIRS} <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    fn, bfn = PAIRS[0][0], PAIRS[0][1]
    cases = [
        ("SELECT * FROM %s('t','v',?,3)" % fn, (q,), "expects 6 arguments, but 4 were provided"),
        ("SELECT * FROM %s('t','v',?,3,7,1)" % fn, (q,), "argument 5 must be of type TEXT (got INTEGER)"),
        ("SELECT * FROM %s('t','v',?,3,'label','x')" % fn, (q,), "argument 6 must be of type INTEGER (got TEXT)"),
        ("SELECT * FROM %s('t','v',?,3,'label',-1)" % fn, (q,), "label -1 is out of range"),
        ("SELECT * FROM %s('t','v',?,3,'label',4294967295)" % fn, (q,), "label 4294967295 is out of range"),
        ("SELECT * FROM %s('t','nope',?,3,'label',1)" % fn, (q,), "unable to retrieve context"),
        ("SELECT * FROM %s('t','v',?,65,'label',1)" % fn, (q,), "k must not exceed 64"),
        ("SELECT * FROM %s('t','v',?,3,'label',1)" % bfn, (q,), "argument 6 must be a BLOB"),
        ("SELECT * FROM %s('t','v',?,3,'label',?)" % bfn, (q, struct.pack("<2q", 1, 2)), "one packed 64-bit label per query"),
        ("SELECT * FROM %s('t','v',?,3,'label',?)" % bfn, (q, struct.pack("<q", 1 << 32)), "label 4294967296 is out of range"),
    ]
    for sql, args, text in cases:
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute(sql, args).fetchall()
        assert text in str(ei.value), (sql, str(ei.value))
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_quantize_scan_labeled('t','v',?,3,'label',1)", (q,)).fetchall()
    assert "Quantization table not found" in str(ei.value)
    assert db.execute("SELECT * FROM %s('t','v',?,0,'label',1)" % fn, (q,)).fetchall() == []          # k = 0: no rows, no device


# ------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric,quantized", [(dg.F32, dg.L2, False), (dg.F32, dg.COSINE, False), (dg.U8, dg.L2, False), (dg.F32, dg.L2, True)])
def test_labeled_equals_the_joined_stream(ext_path, vt, metric, quantized):
    rows = dg.corpus(vt, N, DIM, 11, low_entropy=(vt == dg.U8))
    qs = [dg.query(vt, DIM, 12 + i, low_entropy=(vt == dg.U8)).tobytes() for i in range(5)]
    db = connect(ext_path)
    load_table(db, rows, vt, metric)
    fns = PAIRS[1 if quantized else 0]
    if quantized:
        db.execute("SELECT vector_quantize('t','v')")
    check(db, fns, qs[0])
    check(db, fns, qs[1], labels=(3,), ks=(20,))                 # a second query under the labels already set
    check_batch(db, fns, qs, [6, 0, 3, 99, 0])                   # mixed labels, one nobody has, caller order
    check_batch(db, fns, qs, [2] * 5)
    # ORDER BY distance is consumed
    assert db.execute("SELECT id, distance FROM %s('t','v',?,20,'label',3) ORDER BY distance" % fns[0], (qs[0],)).fetchall() == want(db, fns[2], qs[0], 3, 20)
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra,quantized", [("", False), (",track_changes=1", False), ("", True)])
def test_freshness_update_and_insert(ext_path, extra, quantized):
    rows = dg.corpus(dg.F32, N, DIM, 21)
    q = dg.query(dg.F32, DIM, 22).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2, extra)
    fns = PAIRS[1 if quantized else 0]
    if quantized:
        db.execute("SELECT vector_quantize('t','v')")
    first = single(db, fns[0], q, 20, 3)
    assert first == single(db, fns[0], q, 20, 3)                 # (the second call reuses the labels)
    # an UPDATE of a row's label between two calls is seen by the second call
    best = first[0][0]
    db.execute("UPDATE t SET label = 5 WHERE id = ?", (best,))
    second = single(db, fns[0], q, 20, 3)
    assert best not in [r[0] for r in second] and bits(second) == bits(want(db, fns[2], q, 3, 20))
    assert single(db, fns[0], q, 1, 5)[0][0] == best
    check(db, fns, q, labels=(3, 5), ks=(20,))
    # a label out of range in the column: an error naming the value; put right again, the scan answers
    db.execute("UPDATE t SET label = 4294967295 WHERE id = 2")
    with pytest.raises(sqlite3.OperationalError) as ei:
        single(db, fns[0], q, 20, 3)
    assert "label 4294967295" in str(ei.value) and "out of range" in str(ei.value)
    db.execute("UPDATE t SET label = 0 WHERE id = 2")
    check(db, fns, q, labels=(0, 3), ks=(20,))
    if not quantized:
        # an INSERT between two calls is seen
        db.execute("INSERT INTO t(id, label, v) VALUES (?, 3, ?)", (100000, q))
        got = single(db, fns[0], q, 5, 3)
        assert got[0][0] == 100000
        check(db, fns, q, labels=(3, 0), ks=(20,))
        # another label column: not the labels of the first one
        db.execute("ALTER TABLE t ADD COLUMN other INTEGER")
        db.execute("UPDATE t SET other = id % 4")
        got = db.execute("SELECT id FROM %s('t','v',?,20,'other',1)" % fns[0], (q,)).fetchall()
        assert got and all(r[0] % 4 == 1 for r in got)
        check(db, fns, q, labels=(3,), ks=(20,))
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quantized", [False, True])
def test_out_of_core_table_gives_the_resident_rows(ext_path, quantized, monkeypatch):
    """a table that does not fit the device answers through the slab route with a host-side label compare: the very rows of the resident
    scan, single form and batch form (a label per query), and no row for a label nobody carries"""
    n, dim, k = 3000, 64, 20
    rows = dg.corpus(dg.F32, n, dim, 51)
    qs = [dg.query(dg.F32, dim, 52 + i).tobytes() for i in range(3)]
    fn, bfn, _ = PAIRS[1 if quantized else 0]

    def run():
        db = connect(ext_path)
        db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, label, v BLOB)")
        db.executemany("INSERT INTO t(id, label, v) VALUES (?, ?, ?)", [(j + 1, (j + 1) % 10, rows[j].tobytes()) for j in range(n)])
        db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2')" % dim)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        out = (bits(single(db, fn, qs[0], k, 3)), bits(single(db, fn, qs[0], k, 99)),
               bits(db.execute("SELECT query, id, distance FROM %s('t','v',?,?,'label',?)" % bfn,
                               (b"".join(qs), k, struct.pack("<3q", 7, 99, 2))).fetchall()))
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    assert len(resident[0]) == k and all(r[0] % 10 == 3 for r in resident[0])
    assert resident[1] == []                                         # the label nobody carries: exactly no rows
    assert [(r[0], r[1] % 10) for r in resident[2]] == [(0, 7)] * k + [(2, 2)] * k
    assert ooc == resident

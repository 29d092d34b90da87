"""vector_full_scan_batch_filtered / vector_quantize_scan_batch_filtered(table, column, queries, k, filter) -> (query, id, distance): the
masked batch scans of the C-ABI (vg_scan_topk_batch_masked) behind SQL.  `queries` is the batch functions' argument (a BLOB of nq * dim
elements or a JSON array of arrays), `filter` the filtered functions' (one read-only SELECT yielding rowids, or a BLOB of packed int64
rowids).  The yardstick is the single-query function: for every query of the batch, vector_full_scan_filtered's rows for that query."""
import os
import sqlite3
import struct

import numpy as np
import pytest

import datagen as dg
from test_sql_masked import bits, connect, load_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("vector_full_scan_batch_filtered", "vector_quantize_scan_batch_filtered")


@pytest.fixture(scope="module")
def ext_path():
    import __graft_entry__ as g
    b = g._load_build()
    b.build_gpu_library()
    p = b.build_extension()
    assert p and os.path.exists(p)
    return p[:-3]


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert set(FUNCS) <= mods
    assert {"vector_full_scan_filtered", "vector_quantize_scan_filtered", "vector_full_scan_batch", "vector_quantize_scan_batch"} <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[:2].tobytes()
    f = "SELECT id FROM t"
    for fn in FUNCS:
        cases = [
            ("SELECT * FROM %s('t','v',?,3)" % fn, (q,), "expects 5 arguments, but 4 were provided"),
            ("SELECT * FROM %s('t','v')" % fn, (), "expects 5 arguments, but 2 were provided"),
            ("SELECT * FROM %s(1,'v',?,3,?)" % fn, (q, f), "argument 1 must be of type TEXT (got INTEGER)"),
            ("SELECT * FROM %s('t',2.5,?,3,?)" % fn, (q, f), "argument 2 must be of type TEXT (got REAL)"),
            ("SELECT * FROM %s('t','v',7,3,?)" % fn, (f,), "argument 3 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,'x',?)" % fn, (q, f), "argument 4 must be of type INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','v',?,2.5,?)" % fn, (q, f), "argument 4 must be of type INTEGER (got REAL)"),
            ("SELECT * FROM %s('t','v',?,3,7)" % fn, (q,), "argument 5 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,3,NULL)" % fn, (q,), "filter cannot be NULL"),
            ("SELECT * FROM %s('t','nope',?,3,?)" % fn, (q, f), "unable to retrieve context"),
            ("SELECT * FROM %s('t','v',?,3,?)" % fn, (q[:40], f), "the query batch has 40 bytes, expected a multiple of 32 (dimension 8)"),
            ("SELECT * FROM %s('t','v',?,3,?)" % fn, (b"", f), "the query batch has 0 bytes, expected a multiple of 32 (dimension 8)"),
        ]
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
    fn = FUNCS[0]
    for k, text in ((-1, "k must be positive"), (65, "k must not exceed 64")):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM %s('t','v',?,?,?)" % fn, (q, k, f)).fetchall()
        assert text in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v',?,3,?)" % fn, (q, b"12345")).fetchall()
    assert "multiple of 8" in str(ei.value)
    for text, message in (("DELETE FROM t", "must be a read-only statement"), ("SELECT id FROM t; SELECT 1", "must be a single statement")):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM %s('t','v',?,3,?)" % fn, (q, text)).fetchall()
        assert fn in str(ei.value) and message in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v','[[1,2],[3]]',3,?)" % fn, (f,)).fetchall()          # the JSON parser's own refusal
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v',?,3,?)" % FUNCS[1], (q, f)).fetchall()
    assert "Quantization table not found" in str(ei.value) and FUNCS[1] in str(ei.value)
    # k = 0 or an empty batch: no rows, decided in the extension (no device needed, the filter is not even looked at)
    assert db.execute("SELECT * FROM %s('t','v',?,0,?)" % fn, (q, f)).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v',?,0,'DROP TABLE t')" % fn, (q,)).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v','[]',3,?)" % fn, (f,)).fetchall() == []
    assert db.execute("SELECT count(*) FROM t").fetchone()[0] == 10


def test_scan_without_gpu_is_a_loud_sql_error(ext_path):
    import __graft_entry__ as g
    if g.load_package().device_count() > 0:
        pytest.skip("a GPU is present")
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    for f in ("SELECT id FROM t WHERE tenant = 3", struct.pack("<3q", 1, 2, 3)):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM vector_full_scan_batch_filtered('t','v',?,3,?)", (rows[:2].tobytes(), f)).fetchall()
        assert "no HIP device" in str(ei.value)


# ------------------------------------------------------------------------------------------------- GPU

FILTERS = ["SELECT id FROM t WHERE tenant = 7", "SELECT rowid FROM t WHERE tenant IN (1, 2, 3) AND id > 50", "SELECT id FROM t",
           "SELECT id FROM t WHERE tenant = 77", "SELECT id FROM t WHERE id IN (5, 6, 7)"]


def _singles(db, fn_single, qs, k, flt):
    """(query, id, distance bits) of the single-query filtered function, query by query"""
    out = []
    for i in range(len(qs)):
        out += [(i,) + r for r in bits(db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn_single, (qs[i].tobytes(), k, flt)).fetchall())]
    return out


def _batch(db, fn, queries, k, flt, tail=""):
    return [(r[0], r[1], struct.pack("<d", r[2])) for r in db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?)%s" % (fn, tail), (queries, k, flt)).fetchall()]


def _check(db, fn, fn_single, qs, filters=FILTERS, ks=(1, 20, 64)):
    blob = qs.tobytes()
    js = "[" + ",".join("[" + ",".join(repr(float(x)) for x in q) + "]" for q in qs) + "]"
    for flt in filters:
        ids = [r[0] for r in db.execute(flt).fetchall()]
        for k in ks:
            want = _singles(db, fn_single, qs, k, flt)
            assert _batch(db, fn, blob, k, flt) == want, (fn, flt, k)                                  # a SELECT filter, BLOB queries
            assert _batch(db, fn, js, k, struct.pack("<%dq" % len(ids), *ids)) == want, (fn, flt, k)   # a BLOB filter, JSON queries
            if not ids:
                assert want == []                                                                       # a filter yielding no rows
        assert _batch(db, fn, blob, 0, flt) == []
    # the claimed order is the order the rows come in
    assert _batch(db, fn, blob, 20, filters[0], " ORDER BY query, distance") == _singles(db, fn_single, qs, 20, filters[0])


@pytest.mark.gpu
def test_full_scan_batch_filtered_equals_the_single_filtered_scans(ext_path):
    n, dim = 2000, 48
    rows = dg.corpus(dg.F32, n, dim, 11)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, 5, dim, 12))
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    _check(db, FUNCS[0], "vector_full_scan_filtered", qs)
    # freshness: an INSERT is seen by the next batch - by the filter and by the scan
    db.execute("INSERT INTO t(id, tenant, v) VALUES (?, 7, ?)", (100000, qs[2].tobytes()))
    got = _batch(db, FUNCS[0], qs.tobytes(), 5, FILTERS[0])
    assert [r[:2] for r in got if r[0] == 2][0] == (2, 100000)
    _check(db, FUNCS[0], "vector_full_scan_filtered", qs, FILTERS[:2], (20,))
    db.close()


@pytest.mark.gpu
def test_quantize_scan_batch_filtered_equals_the_single_filtered_scans(ext_path):
    n, dim = 2000, 64
    rows = dg.corpus(dg.F32, n, dim, 31)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, 5, dim, 32))
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    db.execute("SELECT vector_quantize('t','v')")                             # (a uint8 table)
    _check(db, FUNCS[1], "vector_quantize_scan_filtered", qs)
    db.close()


@pytest.mark.gpu
def test_a_second_connection_shares_the_staged_copy_with_another_filter_in_between(ext_path, tmp_path):
    """the mask is state of the staged copy and the copy is shared: every call sets its own mask and scans inside one hold of the lock"""
    n, dim = 2000, 32
    rows = dg.corpus(dg.F32, n, dim, 71)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, 5, dim, 72))
    path = str(tmp_path / "shared.db")
    db = sqlite3.connect(path, isolation_level=None)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", [(i + 1, (i + 1) % 10, rows[i].tobytes()) for i in range(n)])
    db.execute("COMMIT")
    db.close()
    conns = []
    for _ in range(2):
        c = connect(ext_path, path)
        c.execute("SELECT vector_init('t','v','type=FLOAT32,dimension=%d,distance=L2')" % dim)
        conns.append(c)
    filters = ["SELECT id FROM t WHERE tenant = 1", "SELECT id FROM t WHERE tenant = 2"]
    want = [_singles(conns[i], "vector_full_scan_filtered", qs, 20, filters[i]) for i in range(2)]
    assert want[0] != want[1] and len(want[0]) == 100
    for _ in range(3):                                                         # alternating: each call finds the other's mask on the copy
        for i in range(2):
            assert _batch(conns[i], FUNCS[0], qs.tobytes(), 20, filters[i]) == want[i], i
        assert bits(conns[0].execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,20,?)", (qs[0].tobytes(), filters[1])).fetchall()) == \
            [r[1:] for r in want[1] if r[0] == 0]
    for c in conns:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quantized", [False, True])
def test_out_of_core_table_gives_the_resident_rows(ext_path, quantized, monkeypatch):
    """a table that does not fit the device answers through the slab route, query by query: the very rows of the resident scan"""
    n, dim, nq = 3000, 64, 3
    rows = dg.corpus(dg.F32, n, dim, 51)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, nq, dim, 52))
    fn = FUNCS[1 if quantized else 0]
    flt = "SELECT id FROM t WHERE tenant IN (3, 7)"                 # 600 rows

    def run():
        db = connect(ext_path)
        load_table(db, rows, dg.F32, dg.L2)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        ids = [r[0] for r in db.execute(flt).fetchall()]
        blob = struct.pack("<%dq" % len(ids), *ids)
        out = [_batch(db, fn, qs.tobytes(), k, f) for k in (1, 20, 64) for f in (flt, blob)]
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    assert [len(r) for r in resident] == [nq * k for k in (1, 20, 64) for _ in range(2)]
    assert all(r[1] % 10 in (3, 7) for out in resident for r in out)
    assert ooc == resident

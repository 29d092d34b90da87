"""vector_full_scan_filtered / vector_quantize_scan_filtered(table, column, vector, k, filter) -> (id, distance): the masked scans of the
C-ABI (vg_scan_topk_masked) behind SQL.  `filter` is one read-only SELECT yielding rowids, or a BLOB of packed int64 rowids.  The
yardstick is the statement they replace: the stream function's rows WHERE id IN (<filter>) ORDER BY distance, id LIMIT k."""
import json
import os
import sqlite3
import struct
import threading

import numpy as np
import pytest

import datagen as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_OPT = {dg.F32: "FLOAT32", dg.F16: "FLOAT16", dg.BF16: "BFLOAT16", dg.U8: "UINT8", dg.I8: "INT8"}
DIST_OPT = {dg.L2: "L2", dg.SQUARED_L2: "SQUARED_L2", dg.COSINE: "COSINE", dg.DOT: "DOT", dg.L1: "L1"}
FUNCS = ("vector_full_scan_filtered", "vector_quantize_scan_filtered")


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


def load_table(db, rows, vt, metric, extra=""):
    """t(id, tenant, v): ids 1..n (scan order = id order), tenant = id % 10"""
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", [(j + 1, (j + 1) % 10, rows[j].tobytes()) for j in range(rows.shape[0])])
    db.execute("COMMIT")
    db.execute("SELECT vector_init('t', 'v', ?)", ("type=%s,dimension=%d,distance=%s%s" % (TYPE_OPT[vt], rows.shape[1], DIST_OPT[metric], extra),))


def bits(rows):
    return [(i, struct.pack("<d", d)) for i, d in rows]


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert set(FUNCS) <= mods
    assert {"vector_full_scan", "vector_quantize_scan", "vector_full_scan_within", "vector_quantize_scan_within"} <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
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
            ("SELECT * FROM %s('t','v',?,3,?)" % fn, (q[:8], f), "query vector has 8 bytes, expected 32"),
        ]
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
    for k, text in ((-1, "k must be positive"), (65, "k must not exceed 64")):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM vector_full_scan_filtered('t','v',?,?,?)", (q, k, f)).fetchall()
        assert text in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_full_scan_filtered('t','v',?,3,?)", (q, b"12345")).fetchall()
    assert "multiple of 8" in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_quantize_scan_filtered('t','v',?,3,?)", (q, f)).fetchall()
    assert "Quantization table not found" in str(ei.value)
    # k = 0: no rows, decided in the extension (no device needed, the filter is not even looked at)
    assert db.execute("SELECT * FROM vector_full_scan_filtered('t','v',?,0,?)", (q, f)).fetchall() == []
    assert db.execute("SELECT * FROM vector_full_scan_filtered('t','v',?,0,'DROP TABLE t')", (q,)).fetchall() == []
    assert db.execute("SELECT count(*) FROM t").fetchone()[0] == 10


def test_a_refused_filter_runs_nothing(ext_path):
    """a filter that writes, holds two statements or does not parse: a clear error, and the database is as it was"""
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    before = db.execute("SELECT id, tenant, v FROM t ORDER BY id").fetchall()
    cases = [
        ("DELETE FROM t WHERE id = 3", "must be a read-only statement"),
        ("UPDATE t SET tenant = 99", "must be a read-only statement"),
        ("INSERT INTO t(id, tenant, v) VALUES (1000, 1, x'00')", "must be a read-only statement"),
        ("DROP TABLE t", "must be a read-only statement"),
        ("COMMIT", "must be a read-only statement"),
        ("ROLLBACK", "must be a read-only statement"),
        ("BEGIN", "must be a read-only statement"),
        ("PRAGMA user_version = 5", "must be a read-only statement"),
        ("ATTACH ':memory:' AS other", "must be a read-only statement"),
        ("SELECT id FROM t; DELETE FROM t", "must be a single statement"),
        ("SELECT id FROM t; SELECT id FROM t", "must be a single statement"),
        ("SELEC id FROM t", "cannot prepare the filter statement"),
        ("SELECT id FROM no_such_table", "cannot prepare the filter statement"),
        ("", "holds no statement"),
        ("   -- nothing here", "holds no statement"),
    ]
    for fn in FUNCS[:1]:
        for text, message in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute("SELECT * FROM %s('t','v',?,3,?)" % fn, (q, text)).fetchall()
            assert fn in str(ei.value) and message in str(ei.value), (text, str(ei.value))
            assert db.execute("SELECT id, tenant, v FROM t ORDER BY id").fetchall() == before, text
            assert db.in_transaction is False and db.execute("PRAGMA user_version").fetchone()[0] == 0, text
            assert [r[1] for r in db.execute("PRAGMA database_list").fetchall()] == ["main"], text


def test_scan_without_gpu_is_a_loud_sql_error(ext_path):
    import __graft_entry__ as g
    if g.load_package().device_count() > 0:
        pytest.skip("a GPU is present")
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    for f in ("SELECT id FROM t WHERE tenant = 3  ", struct.pack("<3q", 1, 2, 3)):     # (a valid filter, trailing blanks allowed)
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM vector_full_scan_filtered('t','v',?,3,?)", (rows[0].tobytes(), f)).fetchall()
        assert "no HIP device" in str(ei.value)


# ------------------------------------------------------------------------------------------------- GPU

FILTERS = ["SELECT id FROM t WHERE tenant = 7", "SELECT rowid FROM t WHERE tenant IN (1, 2, 3) AND id > 50", "SELECT id FROM t",
           "SELECT id FROM t WHERE tenant = 77", "SELECT id FROM t WHERE id IN (5, 6, 7)",
           "SELECT CASE WHEN id % 2 THEN id ELSE NULL END FROM t", "SELECT id FROM t UNION ALL SELECT id FROM t UNION ALL SELECT 'x' UNION ALL SELECT -5"]


def _want(db, fn_stream, q, flt, k):
    """the statement the masked scan replaces; filters that yield NULLs / text / unknown ids simply match nothing more under IN"""
    return db.execute("SELECT id, distance FROM %s('t','v',?) WHERE id IN (%s) AND distance < 9e999 ORDER BY distance, id LIMIT ?" % (fn_stream, flt), (q, k)).fetchall()


def _check(db, fn, fn_stream, q, filters=FILTERS, ks=(1, 20, 64)):
    for flt in filters:
        for k in ks:
            want = _want(db, fn_stream, q, flt, k)
            got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn, (q, k, flt)).fetchall()
            assert bits(got) == bits(want), (fn, flt, k, got[:3], want[:3])
            ids = [r[0] for r in db.execute(flt).fetchall() if isinstance(r[0], int)]
            blob = struct.pack("<%dq" % len(ids), *ids)
            got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn, (q, k, blob)).fetchall()
            assert bits(got) == bits(want), (fn, flt, k, "blob")
        assert db.execute("SELECT id FROM %s('t','v',?,0,?)" % fn, (q, flt)).fetchall() == []


@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric", [(dg.F32, dg.L2), (dg.F32, dg.COSINE), (dg.U8, dg.L2), (dg.F16, dg.DOT)])
def test_full_scan_filtered_equals_the_filtered_stream(ext_path, vt, metric):
    n, dim = 3001, 48
    rows = dg.corpus(vt, n, dim, 11, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 12, low_entropy=(vt == dg.U8)).tobytes()
    db = connect(ext_path)
    load_table(db, rows, vt, metric)                                          # (the column's default tie_order: the answer does not depend on it)
    _check(db, "vector_full_scan_filtered", "vector_full_scan_stream", q)
    assert len(db.execute("SELECT id FROM vector_full_scan_filtered('t','v',?,20,'SELECT id FROM t WHERE id IN (5,6,7)')", (q,)).fetchall()) == 3
    # freshness: an INSERT is seen by the next scan - by the filter and by the scan
    db.execute("INSERT INTO t(id, tenant, v) VALUES (?, 7, ?)", (100000, q))
    got = db.execute("SELECT id FROM vector_full_scan_filtered('t','v',?,5,?)", (q, FILTERS[0])).fetchall()
    assert got[0] == (100000,)
    _check(db, "vector_full_scan_filtered", "vector_full_scan_stream", q, FILTERS[:3], (20,))
    # ORDER BY distance is consumed; a JSON query
    if vt == dg.U8:
        js = "[" + ",".join(str(int(x)) for x in np.frombuffer(q, dtype=np.uint8)) + "]"
        assert db.execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,20,?) ORDER BY distance", (js, FILTERS[0])).fetchall() == \
            _want(db, "vector_full_scan_stream", q, FILTERS[0], 20)
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("preload", [False, True])
def test_quantize_scan_filtered_equals_the_filtered_stream(ext_path, preload):
    n, dim = 3001, 64
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    db.execute("SELECT vector_quantize('t','v')")
    if preload:
        db.execute("SELECT vector_quantize_preload('t','v')")
    _check(db, "vector_quantize_scan_filtered", "vector_quantize_scan_stream", q)
    db.close()


@pytest.mark.gpu
def test_tracked_changes_update_and_delete(ext_path):
    n, dim = 2500, 32
    rows = dg.corpus(dg.F32, n, dim, 41)
    q = dg.query(dg.F32, dim, 42).tobytes()
    db = connect(ext_path)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", [(i + 1, (i + 1) % 10, rows[i].tobytes()) for i in range(n)])
    db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2,track_changes=1')" % dim)
    _check(db, "vector_full_scan_filtered", "vector_full_scan_stream", q, FILTERS[:3], (20,))
    near = db.execute("SELECT id FROM vector_full_scan_filtered('t','v',?,5,?)", (q, FILTERS[0])).fetchall()
    db.execute("UPDATE t SET v = ? WHERE id = 77", (q,))                       # tenant 7, now at distance 0
    db.execute("DELETE FROM t WHERE id = ?", (near[0][0],))
    got = db.execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,5,?)", (q, FILTERS[0])).fetchall()
    assert got[0] == (77, 0.0) and near[0][0] not in [g[0] for g in got]
    db.execute("UPDATE t SET tenant = 8 WHERE id = 77")                        # leaves the filter, not the table
    got = db.execute("SELECT id FROM vector_full_scan_filtered('t','v',?,5,?)", (q, FILTERS[0])).fetchall()
    assert 77 not in [g[0] for g in got]
    _check(db, "vector_full_scan_filtered", "vector_full_scan_stream", q, FILTERS[:3], (20,))
    db.close()


@pytest.mark.gpu
def test_two_connections_share_one_staged_copy_with_different_filters(ext_path, tmp_path):
    """the mask is state of the staged copy and the copy is shared (vext_shared.inc): set-mask and scan run inside one hold of the lock,
    so connections with different filters, scanning at the same time, each get their own answer"""
    n, dim = 20000, 32
    rows = dg.corpus(dg.F32, n, dim, 71)
    q = dg.query(dg.F32, dim, 72).tobytes()
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
    want = [_want(conns[i], "vector_full_scan_stream", q, filters[i], 20) for i in range(2)]
    assert want[0] != want[1]
    mem = json.loads(conns[1].execute("SELECT vector_gpu_memory('t','v')").fetchone()[0])
    assert mem["column"]["sharers"] == 2, mem
    errors = []

    def worker(i):
        try:
            for _ in range(200):
                got = conns[i].execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,20,?)", (q, filters[i])).fetchall()
                assert bits(got) == bits(want[i]), i
        except Exception as e:                                   # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors[:3]
    for c in conns:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quantized", [False, True])
def test_out_of_core_table_gives_the_resident_rows(ext_path, quantized, monkeypatch):
    n, dim = 3000, 64
    rows = dg.corpus(dg.F32, n, dim, 51)
    q = dg.query(dg.F32, dim, 52).tobytes()
    fn = "vector_quantize_scan_filtered" if quantized else "vector_full_scan_filtered"
    stream = "vector_quantize_scan_stream" if quantized else "vector_full_scan_stream"

    def run():
        db = connect(ext_path)
        load_table(db, rows, dg.F32, dg.L2)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        out = [bits(db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn, (q, k, f)).fetchall()) for f in FILTERS for k in (1, 20, 64)]
        _check(db, fn, stream, q, FILTERS[:4], (20,))
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    assert ooc == resident and len(resident[1]) == 20


@pytest.mark.gpu
def test_several_shards_through_the_extension(ext_path, monkeypatch):
    n, dim = 3001, 32
    rows = dg.corpus(dg.U8, n, dim, 61, low_entropy=True)
    q = dg.query(dg.U8, dim, 62, low_entropy=True).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.U8, dg.L2)
    one = [bits(db.execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,20,?)", (q, f)).fetchall()) for f in FILTERS]
    db.close()
    monkeypatch.setenv("VECTORGPU_DEVICES", "0,0,0")
    monkeypatch.setenv("VECTORGPU_SHARD_ROWS", "40")
    db = connect(ext_path)
    load_table(db, rows, dg.U8, dg.L2)
    assert [bits(db.execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,20,?)", (q, f)).fetchall()) for f in FILTERS] == one
    _check(db, "vector_full_scan_filtered", "vector_full_scan_stream", q, FILTERS[:3], (20,))
    db.close()

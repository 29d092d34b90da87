"""vector_full_scan_within_filtered / vector_quantize_scan_within_filtered(table, column, vector, radius, filter [, limit]) -> (id,
distance) and vector_full_scan_batch_within_filtered / vector_quantize_scan_batch_within_filtered(table, column, queries, radius,
filter [, limit]) -> (query, id, distance): the masked range scans of the C-ABI (vg_scan_within_masked, vg_scan_within_batch_masked)
behind SQL.  The yardstick is the statement they replace: the stream function's rows WHERE id IN (<filter>) AND distance <= r
ORDER BY distance, id [LIMIT n]."""
import json
import os
import shutil
import sqlite3
import struct
import subprocess
import sys
import threading

import pytest

import datagen as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_OPT = {dg.F32: "FLOAT32", dg.F16: "FLOAT16", dg.BF16: "BFLOAT16", dg.U8: "UINT8", dg.I8: "INT8"}
DIST_OPT = {dg.L2: "L2", dg.SQUARED_L2: "SQUARED_L2", dg.COSINE: "COSINE", dg.DOT: "DOT", dg.L1: "L1"}
SINGLE = ("vector_full_scan_within_filtered", "vector_quantize_scan_within_filtered")
BATCH = ("vector_full_scan_batch_within_filtered", "vector_quantize_scan_batch_within_filtered")


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
    return [tuple(r[:-1]) + (struct.pack("<d", r[-1]),) for r in rows]


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert set(SINGLE + BATCH) <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    f = "SELECT id FROM t"
    for fn in SINGLE + BATCH:
        batch = fn in BATCH
        cases = [
            ("SELECT * FROM %s('t','v',?,3.0)" % fn, (q,), "expects 5 or 6 arguments, but 4 were provided"),
            ("SELECT * FROM %s('t','v')" % fn, (), "expects 5 or 6 arguments, but 2 were provided"),
            ("SELECT * FROM %s(1,'v',?,3.0,?)" % fn, (q, f), "argument 1 must be of type TEXT (got INTEGER)"),
            ("SELECT * FROM %s('t',2.5,?,3.0,?)" % fn, (q, f), "argument 2 must be of type TEXT (got REAL)"),
            ("SELECT * FROM %s('t','v',7,3.0,?)" % fn, (f,), "argument 3 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,NULL,?)" % fn, (q, f), "radius cannot be NULL"),
            ("SELECT * FROM %s('t','v',?,x'00',?)" % fn, (q, f),
             "argument 4 must be of type REAL, INTEGER or TEXT (got BLOB)" if batch else "argument 4 must be of type REAL or INTEGER (got BLOB)"),
            ("SELECT * FROM %s('t','v',?,3.0,7)" % fn, (q,), "argument 5 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,3.0,NULL)" % fn, (q,), "filter cannot be NULL"),
            ("SELECT * FROM %s('t','v',?,3.0,?,'x')" % fn, (q, f), "argument 6 must be of type INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','nope',?,3.0,?)" % fn, (q, f), "unable to retrieve context"),
            ("SELECT * FROM %s('t','v',?,3.0,?)" % fn, (q[:8], f), "query vector has 8 bytes, expected " + ("a multiple of 32" if batch else "32")),
            ("SELECT * FROM %s('t','v',?,?,?)" % fn, (q, float("nan"), f), "radius cannot be N"),          # (SQLite binds a NaN as NULL)
        ]
        if not batch:
            cases.append(("SELECT * FROM %s('t','v',?,'[1.0]',?)" % fn, (q, f), "argument 4 must be of type REAL or INTEGER (got TEXT)"))
        if fn.startswith("vector_full"):                                       # (the quantized functions ask for their table first)
            cases += [
                ("SELECT * FROM %s('t','v',?,3.0,?,-1)" % fn, (q, f), "limit must not be negative"),
                ("SELECT * FROM %s('t','v',?,3.0,?)" % fn, (q, b"12345"), "multiple of 8"),
            ]
        if fn == BATCH[0]:
            cases += [
                ("SELECT * FROM %s('t','v',?,'[1.0, 2.0]',?)" % fn, (q, f), "the radius array has 2 values, expected 1 (one per query)"),
                ("SELECT * FROM %s('t','v',?,'[]',?)" % fn, (q, f), "the radius array has 0 values, expected 1"),
                ("SELECT * FROM %s('t','v',?,'[1.0]',?)" % fn, (q + q, f), "the radius array has 1 values, expected 2"),
                ("SELECT * FROM %s('t','v',?,'[nan]',?)" % fn, (q, f), "radius must be a number or a JSON array of numbers"),
                ("SELECT * FROM %s('t','v',?,'1.0',?)" % fn, (q, f), "radius must be a number or a JSON array of numbers"),
            ]
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
        # limit = 0: no rows, decided in the extension (no device needed, the filter is not even looked at)
        if fn.startswith("vector_full"):
            assert db.execute("SELECT * FROM %s('t','v',?,3.0,?,0)" % fn, (q, f)).fetchall() == []
            assert db.execute("SELECT * FROM %s('t','v',?,3.0,'DROP TABLE t',0)" % fn, (q,)).fetchall() == []
    for fn in (SINGLE[1], BATCH[1]):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM %s('t','v',?,3.0,?)" % fn, (q, f)).fetchall()
        assert "Quantization table not found" in str(ei.value)
    assert db.execute("SELECT count(*) FROM t").fetchone()[0] == 10


def test_a_refused_filter_runs_nothing(ext_path):
    """a NULL filter, one that writes, one that holds two statements: a clear error, and the database is as it was"""
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    before = db.execute("SELECT id, tenant, v FROM t ORDER BY id").fetchall()
    cases = [
        ("DELETE FROM t WHERE id = 3", "must be a read-only statement"),
        ("UPDATE t SET tenant = 99", "must be a read-only statement"),
        ("DROP TABLE t", "must be a read-only statement"),
        ("COMMIT", "must be a read-only statement"),
        ("PRAGMA user_version = 5", "must be a read-only statement"),
        ("SELECT id FROM t; DELETE FROM t", "must be a single statement"),
        ("SELECT id FROM t; SELECT id FROM t", "must be a single statement"),
        ("SELEC id FROM t", "cannot prepare the filter statement"),
        ("", "holds no statement"),
    ]
    for fn in (SINGLE[0], BATCH[0]):
        for text, message in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute("SELECT * FROM %s('t','v',?,3.0,?)" % fn, (q, text)).fetchall()
            assert fn in str(ei.value) and message in str(ei.value), (text, str(ei.value))
            assert db.execute("SELECT id, tenant, v FROM t ORDER BY id").fetchall() == before, text
            assert db.in_transaction is False and db.execute("PRAGMA user_version").fetchone()[0] == 0, text
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM %s('t','v',?,3.0,NULL)" % fn, (q,)).fetchall()
        assert "filter cannot be NULL" in str(ei.value)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_an_engine_without_the_masked_range_symbols_names_the_missing_one(ext_path, tmp_path):
    """an older engine (here: the host-memory stub of the sanitizer runs): the extension loads, the reference's functions answer as
    before, the new ones fail with a message naming the missing symbol"""
    stub = str(tmp_path / "stub.so")
    subprocess.run(["gcc", "-O1", "-fPIC", "-shared", "-o", stub, os.path.join(ROOT, "tools", "asan_stub_engine.c"), "-lm"], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", stub], capture_output=True, text=True).stdout
    if "vg_shards_scan_within_masked" in syms or "vg_shards_scan_within_batch_masked" in syms:
        pytest.skip("the stub engine implements the masked range scans")
    first = "vg_shards_set_mask_rowids" if "vg_shards_set_mask_rowids" not in syms else None
    script = (
        "import sqlite3, struct, sys\n"
        "db = sqlite3.connect(':memory:', isolation_level=None)\n"
        "db.enable_load_extension(True)\n"
        "db.load_extension(%r)\n"
        "db.execute('CREATE TABLE t (id INTEGER PRIMARY KEY, v BLOB)')\n"
        "for i in range(1, 9):\n"
        "    db.execute('INSERT INTO t(id, v) VALUES (?, ?)', (i, struct.pack('4f', float(i), 0.0, 0.0, 0.0)))\n"
        "db.execute(\"SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=4,distance=L2')\")\n"
        "q = struct.pack('4f', 0.0, 0.0, 0.0, 0.0)\n"
        "print('TOPK', db.execute(\"SELECT id, distance FROM vector_full_scan('t','v',?,3)\", (q,)).fetchall())\n"
        "for fn in ('vector_full_scan_within_filtered', 'vector_full_scan_batch_within_filtered'):\n"
        "    try:\n"
        "        db.execute(\"SELECT id FROM \" + fn + \"('t','v',?,2.5,'SELECT id FROM t')\", (q,)).fetchall()\n"
        "        print('NEW', fn, 'ok')\n"
        "    except sqlite3.OperationalError as e:\n"
        "        print('NEW', e)\n" % ext_path)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, VECTORGPU_LIB=stub))
    assert out.returncode == 0, out.stderr
    assert "TOPK [(1, 1.0), (2, 2.0), (3, 3.0)]" in out.stdout, out.stdout
    lines = [l for l in out.stdout.splitlines() if l.startswith("NEW")]
    assert len(lines) == 2
    for line, fn, sym in zip(lines, (SINGLE[0], BATCH[0]), ("vg_shards_scan_within_masked", "vg_shards_scan_within_batch_masked")):
        assert fn in line and "lacks symbol " + (first or sym) in line, line


# ------------------------------------------------------------------------------------------------- GPU

FILTERS = ["SELECT id FROM t WHERE tenant = 3", "SELECT rowid FROM t WHERE tenant IN (1, 2, 3) AND id > 50", "SELECT id FROM t",
           "SELECT id FROM t WHERE tenant = 77", "SELECT CASE WHEN id % 2 THEN id ELSE NULL END FROM t"]


def _want(db, stream, q, flt, r, limit=None):
    """the statement the masked range scan replaces"""
    sql = "SELECT id, distance FROM %s('t','v',?) WHERE id IN (%s) AND distance <= ? ORDER BY distance, id" % (stream, flt)
    return db.execute(sql + (" LIMIT %d" % limit if limit is not None else ""), (q, r)).fetchall()


def _radii(db, stream, q, flt="SELECT id FROM t WHERE tenant = 3"):
    d = [r[0] for r in db.execute("SELECT distance FROM %s('t','v',?) WHERE id IN (%s) ORDER BY distance, id" % (stream, flt), (q,)).fetchall()]
    return [d[0], d[5], d[len(d) // 4], 0.5 * (d[20] + d[21]), d[0] - 1.0, 9e999]


def _blob(db, flt):
    ids = [r[0] for r in db.execute(flt).fetchall() if isinstance(r[0], int)]
    return struct.pack("<%dq" % len(ids), *ids)


def _check_single(db, fn, stream, q, filters=FILTERS):
    for r in _radii(db, stream, q):
        for flt in filters:
            want = _want(db, stream, q, flt, r)
            for f in (flt, _blob(db, flt)):                                    # a SELECT filter and a BLOB filter
                got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn, (q, r, f)).fetchall()
                assert bits(got) == bits(want), (fn, flt, r, got[:3], want[:3])
            for limit in (1, 7, len(want) + 3):
                got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?,?)" % fn, (q, r, flt, limit)).fetchall()
                assert bits(got) == bits(_want(db, stream, q, flt, r, limit)), (fn, flt, r, limit)


def _check_batch(db, fn, stream, qs, filters=FILTERS[:3]):
    nq = len(qs)
    blob = b"".join(qs)
    per_query = [_radii(db, stream, qs[i]) for i in range(nq)]
    for flt in filters:
        # a shared radius
        r = per_query[0][2]
        got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?)" % fn, (blob, r, flt)).fetchall()
        for i in range(nq):
            assert bits([g[1:] for g in got if g[0] == i]) == bits(_want(db, stream, qs[i], flt, r)), (fn, flt, "shared", i)
        assert [g[0] for g in got] == sorted(g[0] for g in got)
        # a radius array: one per query, different kinds side by side
        radii = [per_query[i][(i + 1) % 5] for i in range(nq)]
        for f in (flt, _blob(db, flt)):
            got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?)" % fn, (blob, json.dumps(radii), f)).fetchall()
            for i in range(nq):
                assert bits([g[1:] for g in got if g[0] == i]) == bits(_want(db, stream, qs[i], flt, radii[i])), (fn, flt, "array", i)
        got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?,?)" % fn, (blob, json.dumps(radii), flt, 4)).fetchall()
        for i in range(nq):
            assert bits([g[1:] for g in got if g[0] == i]) == bits(_want(db, stream, qs[i], flt, radii[i], 4)), (fn, flt, "limit", i)


@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric", [(dg.F32, dg.L2), (dg.U8, dg.COSINE)])
def test_full_functions_equal_the_filtered_stream(ext_path, vt, metric):
    n, dim = 3001, 48
    rows = dg.corpus(vt, n, dim, 11, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 12, low_entropy=(vt == dg.U8)).tobytes()
    qs = [dg.query(vt, dim, 13 + i, low_entropy=(vt == dg.U8)).tobytes() for i in range(5)]
    db = connect(ext_path)
    load_table(db, rows, vt, metric)
    _check_single(db, SINGLE[0], "vector_full_scan_stream", q)
    _check_batch(db, BATCH[0], "vector_full_scan_stream", qs)
    # freshness: a row inserted into the tenant and a row deleted from it between two calls
    flt = FILTERS[0]
    r = _radii(db, "vector_full_scan_stream", q)[2]
    near = db.execute("SELECT id FROM %s('t','v',?,?,?)" % SINGLE[0], (q, r, flt)).fetchall()
    db.execute("INSERT INTO t(id, tenant, v) VALUES (?, 3, ?)", (100000, q))
    db.execute("DELETE FROM t WHERE id = ?", (near[0][0],))
    got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % SINGLE[0], (q, r, flt)).fetchall()
    assert got[0][0] == 100000 and near[0][0] not in [g[0] for g in got]
    assert bits(got) == bits(_want(db, "vector_full_scan_stream", q, flt, r))
    got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?)" % BATCH[0], (q + qs[0], r, flt)).fetchall()
    assert bits([g[1:] for g in got if g[0] == 0]) == bits(_want(db, "vector_full_scan_stream", q, flt, r))
    assert bits([g[1:] for g in got if g[0] == 1]) == bits(_want(db, "vector_full_scan_stream", qs[0], flt, r))
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric", [(dg.F32, dg.L2), (dg.U8, dg.COSINE)])
def test_quantize_functions_equal_the_filtered_stream(ext_path, vt, metric):
    n, dim = 3001, 64
    rows = dg.corpus(vt, n, dim, 31, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 32, low_entropy=(vt == dg.U8)).tobytes()
    qs = [dg.query(vt, dim, 33 + i, low_entropy=(vt == dg.U8)).tobytes() for i in range(5)]
    db = connect(ext_path)
    load_table(db, rows, vt, metric)
    db.execute("SELECT vector_quantize('t','v')")
    db.execute("SELECT vector_quantize_preload('t','v')")
    _check_single(db, SINGLE[1], "vector_quantize_scan_stream", q, FILTERS[:3])
    _check_batch(db, BATCH[1], "vector_quantize_scan_stream", qs, FILTERS[:2])
    db.close()


@pytest.mark.gpu
def test_two_connections_share_one_staged_copy_with_different_filters(ext_path, tmp_path):
    """the mask is state of the staged copy and the copy is shared: set-mask, scan and fetch run inside one hold of the lock, so
    connections with different filters, scanning at the same time, each get their own tenant's rows"""
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
    r = _radii(conns[0], "vector_full_scan_stream", q, filters[0])[2]
    want = [_want(conns[i], "vector_full_scan_stream", q, filters[i], r) for i in range(2)]
    assert want[0] != want[1] and len(want[0]) > 10 and len(want[1]) > 10
    mem = json.loads(conns[1].execute("SELECT vector_gpu_memory('t','v')").fetchone()[0])
    assert mem["column"]["sharers"] == 2, mem
    errors = []

    def worker(i):
        try:
            for j in range(100):
                if j % 2:
                    got = conns[i].execute("SELECT id, distance FROM %s('t','v',?,?,?)" % SINGLE[0], (q, r, filters[i])).fetchall()
                else:
                    got = [g[1:] for g in conns[i].execute("SELECT query, id, distance FROM %s('t','v',?,?,?)" % BATCH[0], (q, r, filters[i])).fetchall()]
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
def test_out_of_core_table_gives_the_resident_rows(ext_path, monkeypatch):
    n, dim = 3000, 64
    rows = dg.corpus(dg.F32, n, dim, 51)
    q = dg.query(dg.F32, dim, 52).tobytes()
    qs = [dg.query(dg.F32, dim, 53 + i).tobytes() for i in range(3)]

    def run():
        db = connect(ext_path)
        load_table(db, rows, dg.F32, dg.L2)
        _check_single(db, SINGLE[0], "vector_full_scan_stream", q, FILTERS[:2])
        _check_batch(db, BATCH[0], "vector_full_scan_stream", qs, FILTERS[:2])
        r = _radii(db, "vector_full_scan_stream", q)[2]
        out = bits(db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % SINGLE[0], (q, r, FILTERS[0])).fetchall())
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    assert run() == resident and len(resident) > 10

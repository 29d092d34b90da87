"""vector_full_scan_within / vector_quantize_scan_within(table, column, vector, radius [, limit]) -> (id, distance): the range scans of
the C-ABI (vg_scan_within) behind SQL.  The yardstick is the statement they replace - the stream function's rows filtered with
distance <= radius, ordered by (distance, scan position)."""
import os
import shutil
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

import datagen as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_OPT = {dg.F32: "FLOAT32", dg.F16: "FLOAT16", dg.BF16: "BFLOAT16", dg.U8: "UINT8", dg.I8: "INT8"}
DIST_OPT = {dg.L2: "L2", dg.SQUARED_L2: "SQUARED_L2", dg.COSINE: "COSINE", dg.DOT: "DOT", dg.L1: "L1"}


@pytest.fixture(scope="module")
def ext_path():
    import __graft_entry__ as g
    b = g._load_build()
    b.build_gpu_library()
    p = b.build_extension()
    assert p and os.path.exists(p)
    return p[:-3]


def connect(path, file=":memory:"):
    db = sqlite3.connect(file, isolation_level=None)
    db.enable_load_extension(True)
    db.load_extension(path)
    return db


def load_table(db, rows, vt, metric, rowids=None, extra=""):
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, v BLOB)")
    ids = rowids if rowids is not None else range(1, rows.shape[0] + 1)
    db.executemany("INSERT INTO t(id, v) VALUES (?, ?)", [(int(i), rows[j].tobytes()) for j, i in enumerate(ids)])
    db.execute("SELECT vector_init('t', 'v', ?)", ("type=%s,dimension=%d,distance=%s%s" % (TYPE_OPT[vt], rows.shape[1], DIST_OPT[metric], extra),))


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert {"vector_full_scan_within", "vector_quantize_scan_within"} <= mods
    assert {"vector_full_scan", "vector_quantize_scan", "vector_full_scan_stream", "vector_quantize_scan_stream"} <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    for fn in ("vector_full_scan_within", "vector_quantize_scan_within"):
        cases = [
            ("SELECT * FROM %s('t','v',?)" % fn, (q,), "expects 4 or 5 arguments, but 3 were provided"),
            ("SELECT * FROM %s('t','v')" % fn, (), "expects 4 or 5 arguments, but 2 were provided"),
            ("SELECT * FROM %s(1,'v',?,1.0)" % fn, (q,), "argument 1 must be of type TEXT (got INTEGER)"),
            ("SELECT * FROM %s('t',2.5,?,1.0)" % fn, (q,), "argument 2 must be of type TEXT (got REAL)"),
            ("SELECT * FROM %s('t','v',7,1.0)" % fn, (), "argument 3 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,NULL)" % fn, (q,), "radius cannot be NULL"),
            ("SELECT * FROM %s('t','v',?,'far')" % fn, (q,), "argument 4 must be of type REAL or INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','v',?,1.0,'x')" % fn, (q,), "argument 5 must be of type INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','v',?,1.0,2.5)" % fn, (q,), "argument 5 must be of type INTEGER (got REAL)"),
            ("SELECT * FROM %s('t','nope',?,1.0)" % fn, (q,), "unable to retrieve context"),
            ("SELECT * FROM %s('t','v',?,1.0)" % fn, (q[:8],), "query vector has 8 bytes, expected 32"),
        ]
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_full_scan_within('t','v',?,1.0,-1)", (q,)).fetchall()
    assert "limit must not be negative" in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_quantize_scan_within('t','v',?,1.0)", (q,)).fetchall()
    assert "Quantization table not found" in str(ei.value)
    # limit = 0: no rows, decided in the extension (no device needed)
    assert db.execute("SELECT * FROM vector_full_scan_within('t','v',?,1.0,0)", (q,)).fetchall() == []


def test_scan_without_gpu_is_a_loud_sql_error(ext_path):
    import __graft_entry__ as g
    if g.load_package().device_count() > 0:
        pytest.skip("a GPU is present")
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_full_scan_within('t','v',?,3.0)", (rows[0].tobytes(),)).fetchall()
    assert "no HIP device" in str(ei.value)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_an_engine_without_the_range_scan_symbols_still_loads(ext_path, tmp_path):
    """an older engine (here: the host-memory stub of the sanitizer runs, which has no vg_shards_scan_within): the extension loads, the
    reference's functions answer as before, the new ones fail with a message naming the missing symbol"""
    stub = str(tmp_path / "stub.so")
    subprocess.run(["gcc", "-O1", "-fPIC", "-shared", "-o", stub, os.path.join(ROOT, "tools", "asan_stub_engine.c"), "-lm"], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", stub], capture_output=True, text=True).stdout
    if "vg_shards_scan_within" in syms:
        pytest.skip("the stub engine implements the range scans")
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
        "print('STREAM', len(db.execute(\"SELECT id FROM vector_full_scan_stream('t','v',?)\", (q,)).fetchall()))\n"
        "try:\n"
        "    db.execute(\"SELECT id FROM vector_full_scan_within('t','v',?,2.5)\", (q,)).fetchall()\n"
        "    print('WITHIN ok')\n"
        "except sqlite3.OperationalError as e:\n"
        "    print('WITHIN', e)\n" % ext_path)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, VECTORGPU_LIB=stub))
    assert out.returncode == 0, out.stderr
    assert "TOPK [(1, 1.0), (2, 2.0), (3, 3.0)]" in out.stdout and "STREAM 8" in out.stdout, out.stdout
    line = [l for l in out.stdout.splitlines() if l.startswith("WITHIN")][0]
    assert "vector_full_scan_within" in line and "lacks symbol vg_shards_scan_within" in line, line


# ------------------------------------------------------------------------------------------------- GPU

def _want(db, fn_stream, q, radius, limit=None):
    """the statement the range scan replaces: the stream function's rows with distance <= radius, ordered by (distance, scan position)"""
    stream = db.execute("SELECT id, distance FROM %s('t','v',?)" % fn_stream, (q,)).fetchall()
    hits = [(d, pos, i) for pos, (i, d) in enumerate(stream) if d <= radius and d < float("inf")]
    hits.sort()
    out = [(i, d) for d, pos, i in hits]
    return (out if limit is None else out[:limit]), len(stream)


def _radii(db, fn_stream, q):
    d = np.sort(np.array([r[0] for r in db.execute("SELECT distance FROM %s('t','v',?)" % fn_stream, (q,)).fetchall()]))
    d = d[np.isfinite(d)]
    return [float(d[0]), float(d[5]), 0.5 * (float(d[40]) + float(d[41])), float(d[len(d) // 2]), float(d[0]) - 1.0, float(d[-1]), 1e300]


def _check(db, fn, fn_stream, q, radii):
    for radius in radii:
        want, n = _want(db, fn_stream, q, radius)
        got = db.execute("SELECT id, distance FROM %s('t','v',?,?)" % fn, (q, radius)).fetchall()
        assert got == want, (fn, radius, len(got), len(want))
        for limit in (1, 7, len(want), len(want) + 3):
            if limit >= 1:
                got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn, (q, radius, limit)).fetchall()
                assert got == want[:limit], (fn, radius, limit)
        assert db.execute("SELECT id FROM %s('t','v',?,?,0)" % fn, (q, radius)).fetchall() == []
    # an integer radius, a JSON query, ORDER BY distance consumed
    want, _ = _want(db, fn_stream, q, 1000000)
    assert db.execute("SELECT id, distance FROM %s('t','v',?,1000000) ORDER BY distance" % fn, (q,)).fetchall() == want


@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric", [(dg.F32, dg.L2), (dg.F32, dg.COSINE), (dg.U8, dg.L2), (dg.F16, dg.DOT)])
def test_full_scan_within_equals_the_filtered_stream(ext_path, vt, metric):
    n, dim = 3001, 48
    rows = dg.corpus(vt, n, dim, 11, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 12, low_entropy=(vt == dg.U8)).tobytes()
    db = connect(ext_path)
    load_table(db, rows, vt, metric, rowids=[3 * i + 2 for i in range(n)], extra=",tie_order=position")
    radii = _radii(db, "vector_full_scan_stream", q)
    _check(db, "vector_full_scan_within", "vector_full_scan_stream", q, radii)
    # freshness: an INSERT is seen by the next scan
    db.execute("INSERT INTO t(id, v) VALUES (?, ?)", (100000, q))
    _check(db, "vector_full_scan_within", "vector_full_scan_stream", q, radii[:3])
    got = db.execute("SELECT id FROM vector_full_scan_within('t','v',?,?)", (q, radii[3])).fetchall()
    assert (100000,) in got
    db.close()


@pytest.mark.gpu
def test_json_query_and_default_tie_order(ext_path):
    """the order among equal distances is (distance, scan position) whatever tie_order the column runs with (uint8 defaults to reference)"""
    n, dim = 2000, 16
    rows = dg.corpus(dg.U8, n, dim, 21, low_entropy=True)
    qv = dg.query(dg.U8, dim, 22, low_entropy=True)
    db = connect(ext_path)
    load_table(db, rows, dg.U8, dg.L2)
    radius = _radii(db, "vector_full_scan_stream", qv.tobytes())[3]
    want, _ = _want(db, "vector_full_scan_stream", qv.tobytes(), radius)
    assert len(set(d for _, d in want)) < len(want)             # ties are there
    assert db.execute("SELECT id, distance FROM vector_full_scan_within('t','v',?,?)", (qv.tobytes(), radius)).fetchall() == want
    js = "[" + ",".join(str(int(x)) for x in qv) + "]"
    assert db.execute("SELECT id, distance FROM vector_full_scan_within('t','v',?,?)", (js, radius)).fetchall() == want
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("preload", [False, True])
def test_quantize_scan_within_equals_the_filtered_stream(ext_path, preload):
    n, dim = 3001, 64
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    db.execute("SELECT vector_quantize('t','v')")
    if preload:
        db.execute("SELECT vector_quantize_preload('t','v')")
    radii = _radii(db, "vector_quantize_scan_stream", q)
    _check(db, "vector_quantize_scan_within", "vector_quantize_scan_stream", q, radii)
    db.close()


@pytest.mark.gpu
def test_tracked_changes_update_and_delete(ext_path):
    n, dim = 2500, 32
    rows = dg.corpus(dg.F32, n, dim, 41)
    q = dg.query(dg.F32, dim, 42).tobytes()
    db = connect(ext_path)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, v BLOB)")
    db.executemany("INSERT INTO t(id, v) VALUES (?, ?)", [(i + 1, rows[i].tobytes()) for i in range(n)])
    db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2,track_changes=1')" % dim)
    radii = _radii(db, "vector_full_scan_stream", q)
    _check(db, "vector_full_scan_within", "vector_full_scan_stream", q, radii[:4])
    near = db.execute("SELECT id FROM vector_full_scan_within('t','v',?,?)", (q, radii[2])).fetchall()
    db.execute("UPDATE t SET v = ? WHERE id = 77", (q,))                       # now at distance 0
    db.execute("DELETE FROM t WHERE id = ?", (near[0][0],))
    got = db.execute("SELECT id, distance FROM vector_full_scan_within('t','v',?,?)", (q, radii[2])).fetchall()
    assert got[0] == (77, 0.0) and near[0][0] not in [g[0] for g in got]
    _check(db, "vector_full_scan_within", "vector_full_scan_stream", q, radii[:4])
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quantized", [False, True])
def test_out_of_core_table_gives_the_resident_rows(ext_path, quantized, monkeypatch):
    n, dim = 3000, 64
    rows = dg.corpus(dg.F32, n, dim, 51)
    q = dg.query(dg.F32, dim, 52).tobytes()
    fn = "vector_quantize_scan_within" if quantized else "vector_full_scan_within"
    stream = "vector_quantize_scan_stream" if quantized else "vector_full_scan_stream"

    def run():
        db = connect(ext_path)
        load_table(db, rows, dg.F32, dg.L2)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        radii = _radii(db, stream, q)
        out = [db.execute("SELECT id, distance FROM %s('t','v',?,?)" % fn, (q, r)).fetchall() for r in radii]
        out.append(db.execute("SELECT id, distance FROM %s('t','v',?,?,5)" % fn, (q, radii[3])).fetchall())
        _check(db, fn, stream, q, radii[:4])
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    assert ooc == resident and len(resident[3]) > 100 and len(resident[-1]) == 5


@pytest.mark.gpu
def test_several_shards_through_the_extension(ext_path, monkeypatch):
    n, dim = 3001, 32
    rows = dg.corpus(dg.U8, n, dim, 61, low_entropy=True)
    q = dg.query(dg.U8, dim, 62, low_entropy=True).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.U8, dg.L2)
    radii = _radii(db, "vector_full_scan_stream", q)
    one = [db.execute("SELECT id, distance FROM vector_full_scan_within('t','v',?,?)", (q, r)).fetchall() for r in radii]
    db.close()
    monkeypatch.setenv("VECTORGPU_DEVICES", "0,0,0")
    monkeypatch.setenv("VECTORGPU_SHARD_ROWS", "64")
    db = connect(ext_path)
    load_table(db, rows, dg.U8, dg.L2)
    assert [db.execute("SELECT id, distance FROM vector_full_scan_within('t','v',?,?)", (q, r)).fetchall() for r in radii] == one
    _check(db, "vector_full_scan_within", "vector_full_scan_stream", q, radii[:4])
    db.close()

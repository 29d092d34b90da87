"""vector_full_scan_batch_within / vector_quantize_scan_batch_within(table, column, queries, radius [, limit]) -> (query, id, distance): the
batch range scans of the C-ABI (vg_scan_within_batch) behind SQL.  `queries` is the batch functions' argument (a BLOB of nq * dim elements
or a JSON array of arrays), `radius` a number shared by all queries or a JSON array of exactly nq numbers, `limit` is per query.  The
yardstick is the single-query function: for every query of the batch, vector_full_scan_within's rows for that query and radius."""
import os
import sqlite3
import struct

import numpy as np
import pytest

import datagen as dg
from test_sql_masked import DIST_OPT, TYPE_OPT, bits, connect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("vector_full_scan_batch_within", "vector_quantize_scan_batch_within")


@pytest.fixture(scope="module")
def ext_path():
    import __graft_entry__ as g
    b = g._load_build()
    b.build_gpu_library()
    p = b.build_extension()
    assert p and os.path.exists(p)
    return p[:-3]


def load_table(db, rows, vt, metric):
    """t(id, v) with explicit, non-contiguous ids 11, 14, 17, ... (scan order = id order)"""
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, v) VALUES (?, ?)", [(3 * j + 11, rows[j].tobytes()) for j in range(rows.shape[0])])
    db.execute("COMMIT")
    db.execute("SELECT vector_init('t', 'v', ?)", ("type=%s,dimension=%d,distance=%s" % (TYPE_OPT[vt], rows.shape[1], DIST_OPT[metric]),))


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert set(FUNCS) <= mods
    assert {"vector_full_scan_within", "vector_quantize_scan_within", "vector_full_scan_batch", "vector_quantize_scan_batch"} <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[:2].tobytes()
    for fn in FUNCS:
        cases = [
            ("SELECT * FROM %s('t','v',?)" % fn, (q,), "expects 4 or 5 arguments, but 3 were provided"),
            ("SELECT * FROM %s('t','v')" % fn, (), "expects 4 or 5 arguments, but 2 were provided"),
            ("SELECT * FROM %s(1,'v',?,1.0)" % fn, (q,), "argument 1 must be of type TEXT (got INTEGER)"),
            ("SELECT * FROM %s('t',2.5,?,1.0)" % fn, (q,), "argument 2 must be of type TEXT (got REAL)"),
            ("SELECT * FROM %s('t','v',7,1.0)" % fn, (), "argument 3 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,NULL)" % fn, (q,), "radius cannot be NULL"),
            ("SELECT * FROM %s('t','v',?,?)" % fn, (q, b"ab"), "argument 4 must be of type REAL, INTEGER or TEXT (got BLOB)"),
            ("SELECT * FROM %s('t','v',?,1.0,'x')" % fn, (q,), "argument 5 must be of type INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','v',?,1.0,2.5)" % fn, (q,), "argument 5 must be of type INTEGER (got REAL)"),
            ("SELECT * FROM %s('t','nope',?,1.0)" % fn, (q,), "unable to retrieve context"),
            ("SELECT * FROM %s('t','v',?,1.0)" % fn, (q[:40],), "query vector has 40 bytes, expected a multiple of 32 (dimension 8)"),
            ("SELECT * FROM %s('t','v',?,1.0)" % fn, (b"",), "query vector has 0 bytes, expected a multiple of 32 (dimension 8)"),
        ]
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
    fn = FUNCS[0]
    for radius, text in (("[1.0]", "the radius array has 1 values, expected 2 (one per query)"),
                         ("[1.0, 2.0, 3.0]", "the radius array has 3 values, expected 2 (one per query)"),
                         ("[]", "the radius array has 0 values, expected 2 (one per query)"),
                         ("1.0", "radius must be a number or a JSON array of numbers"),
                         ("[1.0, x]", "radius must be a number or a JSON array of numbers"),
                         ("[1.0 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[1.0, 2.0] 3", "radius must be a number or a JSON array of numbers"),
                         ("[1.0, 2.0,]", "radius must be a number or a JSON array of numbers"),      # JSON numbers only
                         ("[,1.0, 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[0x10, 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[inf, 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[+1.0, 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[1., 2.0]", "radius must be a number or a JSON array of numbers"),
                         ("[1.0, nan]", "radius must be a number or a JSON array of numbers")):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM %s('t','v',?,?)" % fn, (q, radius)).fetchall()
        assert fn in str(ei.value) and text in str(ei.value), (radius, str(ei.value))
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v',?,1.0,-1)" % fn, (q,)).fetchall()
    assert "limit must not be negative" in str(ei.value)
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v','[[1,2],[3]]',1.0)" % fn).fetchall()                # the JSON parser's own refusal
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM %s('t','v',?,1.0)" % FUNCS[1], (q,)).fetchall()
    assert "Quantization table not found" in str(ei.value) and FUNCS[1] in str(ei.value)
    # limit = 0 or an empty batch: no rows, decided in the extension (no device needed)
    assert db.execute("SELECT * FROM %s('t','v',?,1.0,0)" % fn, (q,)).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v','[]',1.0)" % fn).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v','[]','[]')" % fn).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v','[]',' [ ] ')" % fn).fetchall() == []
    assert db.execute("SELECT * FROM %s('t','v',?,' [ -1.5e+0 ,2E-1 ] ',0)" % fn, (q,)).fetchall() == []    # (well-formed; limit 0: no rows, no device)


def test_scan_without_gpu_is_a_loud_sql_error(ext_path):
    import __graft_entry__ as g
    if g.load_package().device_count() > 0:
        pytest.skip("a GPU is present")
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    for radius in (1.0, "[1.0, 2.0]"):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute("SELECT * FROM vector_full_scan_batch_within('t','v',?,?)", (rows[:2].tobytes(), radius)).fetchall()
        assert "no HIP device" in str(ei.value)


# ------------------------------------------------------------------------------------------------- GPU

def _singles(db, fn_single, qs, radii, limit=None):
    """(query, id, distance bits) of the single-query within function, query by query"""
    out = []
    for i in range(len(qs)):
        if limit is None:
            got = db.execute("SELECT id, distance FROM %s('t','v',?,?)" % fn_single, (qs[i].tobytes(), radii[i])).fetchall()
        else:
            got = db.execute("SELECT id, distance FROM %s('t','v',?,?,?)" % fn_single, (qs[i].tobytes(), radii[i], limit)).fetchall()
        out += [(i,) + r for r in bits(got)]
    return out


def _batch(db, fn, queries, radius, limit=None, tail=""):
    if limit is None:
        got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?)%s" % (fn, tail), (queries, radius)).fetchall()
    else:
        got = db.execute("SELECT query, id, distance FROM %s('t','v',?,?,?)%s" % (fn, tail), (queries, radius, limit)).fetchall()
    return [(r[0], r[1], struct.pack("<d", r[2])) for r in got]


def _check(db, fn, fn_single, qs):
    nq = len(qs)
    blob = qs.tobytes()
    js = "[" + ",".join("[" + ",".join(repr(float(x)) for x in q) + "]" for q in qs) + "]"
    # radii from the single stream function's distances: a few rows, many rows, none, all - different per query
    stream = fn_single.replace("_within", "_stream")
    per_query = []
    for i in range(nq):
        d = np.sort(np.array([r[0] for r in db.execute("SELECT distance FROM %s('t','v',?)" % stream, (qs[i].tobytes(),)).fetchall()]))
        per_query.append([float(d[3 + i]), float(d[40]), float(d[0]) - 1.0, float(d[-1]), 0.5 * (float(d[7]) + float(d[8]))])
    shared = per_query[0][1]
    # a shared radius: REAL, and INTEGER where it is one
    want = _singles(db, fn_single, qs, [shared] * nq)
    assert len(want) >= 40 and _batch(db, fn, blob, shared) == want
    assert _batch(db, fn, js, shared) == want
    big = int(per_query[0][3]) + 1
    assert _batch(db, fn, blob, big) == _singles(db, fn_single, qs, [big] * nq)
    for limit in (1, 7, 1000):
        assert _batch(db, fn, blob, shared, limit) == _singles(db, fn_single, qs, [shared] * nq, limit), limit
    # per-query radii: a JSON array of exactly nq numbers
    for rnd in range(5):
        radii = [per_query[i][(i + rnd) % 5] for i in range(nq)]
        arr = "[" + ", ".join(repr(r) for r in radii) + "]"
        want = _singles(db, fn_single, qs, radii)
        assert _batch(db, fn, blob, arr) == want, rnd
        assert _batch(db, fn, js, arr) == want, rnd
        for limit in (1, 5):
            assert _batch(db, fn, blob, arr, limit) == _singles(db, fn_single, qs, radii, limit), (rnd, limit)
        assert _batch(db, fn, blob, arr, 0) == []
    # the claimed order is the order the rows come in, and claiming it needs no sorter
    radii = [per_query[i][1] for i in range(nq)]
    arr = "[" + ", ".join(repr(r) for r in radii) + "]"
    want = _singles(db, fn_single, qs, radii)
    assert [r[0] for r in want] == sorted(r[0] for r in want) and len(set(r[0] for r in want)) == nq
    assert all(r[1] >= 11 and (r[1] - 11) % 3 == 0 for r in want)                        # the table's own ids
    for tail in (" ORDER BY query, distance", " ORDER BY query"):
        assert _batch(db, fn, blob, arr, tail=tail) == want
        plan = db.execute("EXPLAIN QUERY PLAN SELECT query, id, distance FROM %s('t','v',?,?)%s" % (fn, tail), (blob, arr)).fetchall()
        assert not any("TEMP B-TREE" in str(r[-1]).upper() for r in plan), plan
    plan = db.execute("EXPLAIN QUERY PLAN SELECT query, id, distance FROM %s('t','v',?,?) ORDER BY distance" % fn, (blob, arr)).fetchall()
    assert any("TEMP B-TREE" in str(r[-1]).upper() for r in plan), plan                  # (an order it does not produce is not claimed)


@pytest.mark.gpu
def test_full_scan_batch_within_equals_the_single_within_scans(ext_path):
    n, dim = 300, 16
    rows = dg.corpus(dg.F32, n, dim, 11)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, 5, dim, 12))
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    _check(db, FUNCS[0], "vector_full_scan_within", qs)
    # freshness: an INSERT is seen by the next batch
    db.execute("INSERT INTO t(id, v) VALUES (?, ?)", (100000, qs[2].tobytes()))
    got = _batch(db, FUNCS[0], qs.tobytes(), "[0.0, 0.0, 0.0, 0.0, 0.0]")
    assert [r[:2] for r in got] == [(2, 100000)]
    db.close()


@pytest.mark.gpu
def test_quantize_scan_batch_within_equals_the_single_within_scans(ext_path):
    n, dim = 300, 16
    rows = dg.corpus(dg.F32, n, dim, 31)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, 5, dim, 32))
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    db.execute("SELECT vector_quantize('t','v')")                             # (a uint8 table)
    _check(db, FUNCS[1], "vector_quantize_scan_within", qs)
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quantized", [False, True])
def test_out_of_core_table_gives_the_resident_rows(ext_path, quantized, monkeypatch):
    """a table that does not fit the device answers through the slab route, query by query: the very rows of the resident scan"""
    n, dim, nq = 3000, 64, 3
    rows = dg.corpus(dg.F32, n, dim, 51)
    qs = np.ascontiguousarray(dg.corpus(dg.F32, nq, dim, 52))
    fn = FUNCS[1 if quantized else 0]
    stream = "vector_quantize_scan_stream" if quantized else "vector_full_scan_stream"

    def run():
        db = connect(ext_path)
        db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, v BLOB)")
        db.executemany("INSERT INTO t(id, v) VALUES (?, ?)", [(j + 1, rows[j].tobytes()) for j in range(n)])
        db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2')" % dim)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        radii = []
        for i in range(nq):                               # a radius per query: its 10th, 25th, 40th smallest distance
            d = np.sort(np.array([r[0] for r in db.execute("SELECT distance FROM %s('t','v',?)" % stream, (qs[i].tobytes(),)).fetchall()]))
            radii.append(float(d[9 + 15 * i]))
        arr = "[" + ", ".join(repr(r) for r in radii) + "]"
        out = (_batch(db, fn, qs.tobytes(), arr), _batch(db, fn, qs.tobytes(), arr, 5))
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    for q in range(nq):
        assert sum(1 for r in resident[0] if r[0] == q) >= 10, q
    assert [r[0] for r in resident[1]] == [0] * 5 + [1] * 5 + [2] * 5
    assert ooc == resident

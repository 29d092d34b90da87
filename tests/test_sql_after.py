"""vector_full_scan_after / vector_quantize_scan_after(table, column, vector, k, after_distance, after_rowid) and the _filtered_after
forms (..., k, filter, after_distance, after_rowid) -> (id, distance): the paged scans of the C-ABI (vg_scan_topk_after) behind SQL.
The cursor is the previous page's last (distance, id); both NULL = the first page.  The yardstick is the statement a paging loop
replaces: the stream function's rows [WHERE id IN (<filter>)] ORDER BY distance, id."""
import json
import sqlite3
import threading

import numpy as np
import pytest

import datagen as dg
from test_sql_masked import bits, connect, ext_path, load_table     # noqa: F401  (ext_path is a fixture)

PLAIN = ("vector_full_scan_after", "vector_quantize_scan_after")
FILTERED = ("vector_full_scan_filtered_after", "vector_quantize_scan_filtered_after")


# ------------------------------------------------------------------------------------------------- CPU

def test_modules_are_registered_and_arguments_are_checked_without_a_device(ext_path):
    db = connect(ext_path)
    mods = set(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall())
    assert set(PLAIN + FILTERED) <= mods
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    q = rows[0].tobytes()
    f = "SELECT id FROM t"
    for fn in PLAIN + FILTERED:
        filt = fn in FILTERED
        head = "'t','v',?,3" + (",?" if filt else "")           # up to k (and the filter)
        hargs = (q, f) if filt else (q,)
        nargs = 7 if filt else 6
        a = nargs - 1                                            # number of the after_distance argument
        cases = [
            ("SELECT * FROM %s('t','v',?,3)" % fn, (q,), "expects %d arguments, but 4 were provided" % nargs),
            ("SELECT * FROM %s(%s,1.5)" % (fn, head), hargs, "expects %d arguments, but %d were provided" % (nargs, nargs - 1)),
            ("SELECT * FROM %s(%s,NULL,5)" % (fn, head), hargs, "must both be NULL (the first page) or both be given"),
            ("SELECT * FROM %s(%s,1.5,NULL)" % (fn, head), hargs, "must both be NULL (the first page) or both be given"),
            ("SELECT * FROM %s(%s,'x',5)" % (fn, head), hargs, "argument %d must be a number (got TEXT)" % a),
            ("SELECT * FROM %s(%s,x'00',5)" % (fn, head), hargs, "argument %d must be a number (got BLOB)" % a),
            ("SELECT * FROM %s(%s,1.5,'y')" % (fn, head), hargs, "argument %d must be of type INTEGER (got TEXT)" % (a + 1)),
            ("SELECT * FROM %s(%s,1.5,2.5)" % (fn, head), hargs, "argument %d must be of type INTEGER (got REAL)" % (a + 1)),
            ("SELECT * FROM %s(1,'v',?,3%s,NULL,NULL)" % (fn, ",?" if filt else ""), hargs, "argument 1 must be of type TEXT (got INTEGER)"),
            ("SELECT * FROM %s('t','v',7,3%s,NULL,NULL)" % (fn, ",?" if filt else ""), hargs[1:], "argument 3 must be of type TEXT or BLOB (got INTEGER)"),
            ("SELECT * FROM %s('t','v',?,'x'%s,NULL,NULL)" % (fn, ",?" if filt else ""), hargs, "argument 4 must be of type INTEGER (got TEXT)"),
            ("SELECT * FROM %s('t','nope',?,3%s,NULL,NULL)" % (fn, ",?" if filt else ""), hargs, "unable to retrieve context"),
        ]
        if filt:
            cases.append(("SELECT * FROM %s('t','v',?,3,NULL,NULL,NULL)" % fn, (q,), "filter cannot be NULL"))
        for sql, args, text in cases:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute(sql, args).fetchall()
            assert fn in str(ei.value) and text in str(ei.value), (sql, str(ei.value))
        if fn.startswith("vector_full"):
            for k, text in ((-1, "k must be positive"), (0, "k must be positive"), (65, "k must not exceed 64")):
                with pytest.raises(sqlite3.OperationalError) as ei:
                    db.execute("SELECT * FROM %s('t','v',?,?%s,NULL,NULL)" % (fn, ",?" if filt else ""), (q, k) + hargs[1:]).fetchall()
                assert text in str(ei.value), (fn, k, str(ei.value))
        else:
            with pytest.raises(sqlite3.OperationalError) as ei:
                db.execute("SELECT * FROM %s(%s,NULL,NULL)" % (fn, head), hargs).fetchall()
            assert "Quantization table not found" in str(ei.value)
    # NaN cannot be written in SQL (it reads as NULL): with a rowid given that is "exactly one NULL"
    with pytest.raises(sqlite3.OperationalError) as ei:
        db.execute("SELECT * FROM vector_full_scan_after('t','v',?,3,?,5)", (q, float("nan"))).fetchall()
    assert "must both be NULL" in str(ei.value)


def test_scan_without_gpu_is_a_loud_sql_error(ext_path):
    import __graft_entry__ as g
    if g.load_package().device_count() > 0:
        pytest.skip("a GPU is present")
    db = connect(ext_path)
    rows = dg.corpus(dg.F32, 10, 8, 1)
    load_table(db, rows, dg.F32, dg.L2)
    for sql, args in (("SELECT * FROM vector_full_scan_after('t','v',?,3,NULL,NULL)", (rows[0].tobytes(),)),
                      ("SELECT * FROM vector_full_scan_filtered_after('t','v',?,3,'SELECT id FROM t',0.5,3)", (rows[0].tobytes(),))):
        with pytest.raises(sqlite3.OperationalError) as ei:
            db.execute(sql, args).fetchall()
        assert "no HIP device" in str(ei.value)


# ------------------------------------------------------------------------------------------------- GPU

def _pages(db, fn, q, k, flt=None, limit_pages=None):
    """the paging loop: the cursor comes from the previous page's last row"""
    out, after, pages = [], (None, None), 0
    while limit_pages is None or pages < limit_pages:
        if flt is None:
            page = db.execute("SELECT id, distance FROM %s('t','v',?,?,?,?)" % fn, (q, k) + after).fetchall()
        else:
            page = db.execute("SELECT id, distance FROM %s('t','v',?,?,?,?,?)" % fn, (q, k, flt) + after).fetchall()
        pages += 1
        out += page
        if len(page) < k:
            break
        after = (page[-1][1], page[-1][0])
    return out


def _stream(db, stream, q, flt=None):
    where = "distance < 9e999" + (" AND id IN (%s)" % flt if flt else "")
    return db.execute("SELECT id, distance FROM %s('t','v',?) WHERE %s ORDER BY distance, id" % (stream, where), (q,)).fetchall()


@pytest.mark.gpu
@pytest.mark.parametrize("vt,metric", [(dg.F32, dg.L2), (dg.U8, dg.L2)])
def test_paging_loop_reproduces_the_ordered_stream(ext_path, vt, metric):
    n, dim = 3000, 48
    rows = dg.corpus(vt, n, dim, 11, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 12, low_entropy=(vt == dg.U8)).tobytes()
    db = connect(ext_path)
    load_table(db, rows, vt, metric)
    want = _stream(db, "vector_full_scan_stream", q)
    assert len(want) == n
    if vt == dg.U8:
        d = [w[1] for w in want]
        assert len(set(d)) < len(d), "the low-entropy table is there for equal distances"
    for k in (64, 37):
        assert bits(_pages(db, "vector_full_scan_after", q, k)) == bits(want), k
    # an explicit cursor; ORDER BY distance is consumed
    mid = want[1234]
    got = db.execute("SELECT id, distance FROM vector_full_scan_after('t','v',?,20,?,?) ORDER BY distance", (q, mid[1], mid[0])).fetchall()
    assert bits(got) == bits(want[1235:1255])
    assert db.execute("SELECT id FROM vector_full_scan_after('t','v',?,20,?,?)", (q, want[-1][1], want[-1][0])).fetchall() == []
    # with a SELECT filter
    flt = "SELECT id FROM t WHERE tenant IN (3, 7)"
    wantf = _stream(db, "vector_full_scan_stream", q, flt)
    assert len(wantf) == 600
    assert bits(_pages(db, "vector_full_scan_filtered_after", q, 64, flt)) == bits(wantf)
    # the cursor's row need not pass the filter
    other = next(w for w in want[500:] if w[0] % 10 not in (3, 7))
    got = db.execute("SELECT id, distance FROM vector_full_scan_filtered_after('t','v',?,20,?,?,?)", (q, flt, other[1], other[0])).fetchall()
    behind = [w for w in wantf if (w[1], w[0]) > (other[1], other[0])][:20]
    assert bits(got) == bits(behind)
    db.close()


@pytest.mark.gpu
def test_quantized_table_paging_loop(ext_path):
    n, dim = 3000, 64
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32).tobytes()
    db = connect(ext_path)
    load_table(db, rows, dg.F32, dg.L2)
    db.execute("SELECT vector_quantize('t','v')")
    want = _stream(db, "vector_quantize_scan_stream", q)
    assert bits(_pages(db, "vector_quantize_scan_after", q, 64)) == bits(want)
    flt = "SELECT id FROM t WHERE tenant = 7"
    assert bits(_pages(db, "vector_quantize_scan_filtered_after", q, 20, flt)) == bits(_stream(db, "vector_quantize_scan_stream", q, flt))
    db.close()


@pytest.mark.gpu
def test_delete_of_the_cursor_row_between_two_pages(ext_path):
    n, dim = 2500, 32
    rows = dg.corpus(dg.F32, n, dim, 41)
    q = dg.query(dg.F32, dim, 42).tobytes()
    db = connect(ext_path)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", [(i + 1, (i + 1) % 10, rows[i].tobytes()) for i in range(n)])
    db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2,track_changes=1')" % dim)
    first = db.execute("SELECT id, distance FROM vector_full_scan_after('t','v',?,20,NULL,NULL)", (q,)).fetchall()
    before = _stream(db, "vector_full_scan_stream", q)
    assert bits(first) == bits(before[:20])
    cursor = first[-1]
    db.execute("DELETE FROM t WHERE id = ?", (cursor[0],))                     # the cursor's own row ...
    db.execute("DELETE FROM t WHERE id = ?", (before[21][0],))                 # ... and one of the coming page
    second = db.execute("SELECT id, distance FROM vector_full_scan_after('t','v',?,20,?,?)", (q, cursor[1], cursor[0])).fetchall()
    after = _stream(db, "vector_full_scan_stream", q)
    assert len(after) == n - 2
    assert bits(second) == bits(after[19:39])                                  # continues where it should: nothing repeated, nothing skipped
    assert not set(r[0] for r in second) & set(r[0] for r in first)
    db.close()


@pytest.mark.gpu
def test_two_connections_share_one_staged_copy(ext_path, tmp_path):
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
    want = [_stream(conns[i], "vector_full_scan_stream", q, filters[i])[:200] for i in range(2)]
    assert want[0] != want[1]
    mem = json.loads(conns[1].execute("SELECT vector_gpu_memory('t','v')").fetchone()[0])
    assert mem["column"]["sharers"] == 2, mem
    errors = []

    def worker(i):
        try:
            for _ in range(10):                                  # ten walks of ten pages, the other connection's filter in between
                got = _pages(conns[i], "vector_full_scan_filtered_after", q, 20, filters[i], limit_pages=10)
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
def test_out_of_core_table_gives_the_resident_pages(ext_path, quantized, monkeypatch):
    """a table that does not fit the device answers through the slab route: three pages of 20 from the first page on are the first 60
    rows of the ordered stream (of the filtered stream), and the very rows of the resident scan"""
    n, dim = 3000, 64
    rows = dg.corpus(dg.F32, n, dim, 51)
    q = dg.query(dg.F32, dim, 52).tobytes()
    kind = "quantize" if quantized else "full"
    flt = "SELECT id FROM t WHERE tenant IN (3, 7)"

    def run():
        db = connect(ext_path)
        load_table(db, rows, dg.F32, dg.L2)
        if quantized:
            db.execute("SELECT vector_quantize('t','v')")
        out = (bits(_pages(db, "vector_%s_scan_after" % kind, q, 20, limit_pages=3)),
               bits(_pages(db, "vector_%s_scan_filtered_after" % kind, q, 20, flt, limit_pages=3)),
               bits(_stream(db, "vector_%s_scan_stream" % kind, q)[:60]),
               bits(_stream(db, "vector_%s_scan_stream" % kind, q, flt)[:60]))
        db.close()
        return out

    resident = run()
    monkeypatch.setenv("VECTORGPU_HBM_LIMIT", "16K")
    ooc = run()
    assert len(resident[0]) == 60 and len(resident[1]) == 60
    assert resident[0] == resident[2] and resident[1] == resident[3]
    assert ooc[0] == ooc[2] and ooc[1] == ooc[3]
    assert ooc == resident

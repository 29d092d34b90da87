"""The SQL surface of the extension's 26 table-valued functions, pinned against a literal table: module names, (column, hidden) lists,
the idxNum each plan reports and which ORDER BY each module claims.  No device and no table is needed: xFilter is never called, the
statements are only prepared (EXPLAIN QUERY PLAN)."""
import os
import sqlite3

import pytest

# the four column layouts behind the hidden arguments; "+" marks a hidden column
REF = "+tbl +vector +k +memidx id distance"                # the reference's functions: their four arguments land in these four columns
SINGLE = "id distance +tbl +col +vector "
BATCH = "query id distance +tbl +col +queries "

# module -> (columns, arguments of a full call, idxNum, sorter needed for ORDER BY distance [, ORDER BY query, ORDER BY query, distance])
SURFACE = {
    "scan": (REF, 4, 1, (False,)),
    "scan_stream": (REF, 3, 0, (True,)),
    "scan_batch": (REF + " query", 4, 2, (True, False, False)),
    "scan_within": (SINGLE + "+radius +lim", 5, 1, (False,)),
    "scan_filtered": (SINGLE + "+k +filter", 5, 1, (False,)),
    "scan_within_filtered": (SINGLE + "+radius +filter +lim", 6, 1, (False,)),
    "scan_after": (SINGLE + "+k +after_distance +after_rowid", 6, 1, (False,)),
    "scan_filtered_after": (SINGLE + "+k +filter +after_distance +after_rowid", 7, 1, (False,)),
    "scan_labeled": (SINGLE + "+k +label_column +label", 6, 1, (False,)),
    "scan_batch_within": (BATCH + "+radius +lim", 5, 4, (True, False, False)),
    "scan_batch_filtered": (BATCH + "+k +filter", 5, 3, (True, False, False)),
    "scan_batch_within_filtered": (BATCH + "+radius +filter +lim", 6, 4, (True, False, False)),
    "scan_batch_labeled": (BATCH + "+k +label_column +labels", 6, 3, (True, False, False)),
}
MODULES = sorted("vector_%s_%s" % (kind, form) for kind in ("full", "quantize") for form in SURFACE)
ORDERS = (" ORDER BY distance", " ORDER BY query", " ORDER BY query, distance")


@pytest.fixture(scope="module")
def db():
    import __graft_entry__ as g
    p = g._load_build().build_extension()
    assert p and os.path.exists(p)
    con = sqlite3.connect(":memory:", isolation_level=None)
    con.enable_load_extension(True)
    con.load_extension(p[:-3])
    yield con
    con.close()


def test_the_26_modules_are_registered(db):
    assert len(MODULES) == 26
    assert sorted(r[0] for r in db.execute("SELECT name FROM pragma_module_list WHERE name LIKE 'vector_%'").fetchall()) == MODULES


@pytest.mark.parametrize("module", MODULES)
def test_columns_plan_and_order_claims(db, module):
    columns, nargs, idx_num, sorts = SURFACE[module.split("_", 2)[2]]
    want = [(c.lstrip("+"), int(c.startswith("+"))) for c in columns.split()]
    assert [(r[1], r[6]) for r in db.execute("SELECT * FROM pragma_table_xinfo(?)", (module,)).fetchall()] == want
    call = "SELECT * FROM %s(%s)" % (module, ",".join("?" * nargs))

    def plan(tail=""):
        return [str(r[-1]) for r in db.execute("EXPLAIN QUERY PLAN " + call + tail, (None,) * nargs).fetchall()]

    scans = [line for line in plan() if "VIRTUAL TABLE INDEX" in line]
    assert len(scans) == 1 and module in scans[0] and scans[0].endswith("VIRTUAL TABLE INDEX %d:" % idx_num), scans
    assert len(sorts) == (3 if ("query", 0) in want else 1)
    for tail, sorter in zip(ORDERS, sorts):
        assert any("USE TEMP B-TREE FOR ORDER BY" in line for line in plan(tail)) == sorter, (module, tail)

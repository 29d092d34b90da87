/* vext_batch_within_masked.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * masked batch range scans: vector_full_scan_batch_within_filtered / vector_quantize_scan_batch_within_filtered(table, column, queries,
 * radius, filter [, limit]) -> (query, id, distance): for every query of the batch every row among those the filter names whose
 * distance is <= that query's radius, ordered by query number (0-based), then (distance, scan position).  `queries` and `radius` are
 * the batch range functions' arguments (vext_batch.inc, vext_batch_within.inc: radius a REAL / INTEGER shared by all queries, or a JSON
 * array of exactly nq numbers), `filter` the masked functions' (vext_masked.inc), `limit` is per query.  Each query's rows are what
 * vector_full_scan_within_filtered returns for it and its radius.  Everything behind the arguments - staging, the one hold of the lock
 * around mask + scan + fetch, the out-of-core route - is wmasked_run (vext_within_masked.inc); cursor, columns and index plan are the
 * batch range functions'.
 */
static int bwmasked_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, radius hidden, filter hidden, lim hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int bwmasked_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return wmasked_plan(v, info, bwithin_best_index, BWCOL_TBL, BWMCOL_LIMIT); }

static int bwmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->stream_pos = 0;
    c->stream_n = 0;
    int rc = wmasked_arg_types(vt, fname, argc, argv, 1);
    if (rc != SQLITE_OK) return rc;
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
    table_ctx *t = context_lookup(vt->ctx, tbl, col);
    if (!t) return vtab_error(&vt->base, "%s: unable to retrieve context.", fname);
    const int dim = t->opt.v_dim;
    const int64_t qrow = (int64_t)dim * elem_size(t->opt.v_type);
    if (sqlite3_value_type(argv[2]) == SQLITE_BLOB) {
        const int64_t bytes = sqlite3_value_bytes(argv[2]);
        if (bytes == 0 || bytes % qrow != 0)
            return vtab_error(&vt->base, "%s: query vector has %lld bytes, expected a multiple of %lld (dimension %d).", fname, (long long)bytes, (long long)qrow, dim);
    }
    const uint8_t *queries = NULL;
    void *owned = NULL;
    double *radii = NULL;
    int nq = 0;
    rc = batch_queries_arg(vt, fname, t, argv[2], &queries, &owned, &nq);
    if (rc != SQLITE_OK) return rc;
    if (quantized && (rc = wmasked_quant_table_check(vt, fname, tbl, col)) != SQLITE_OK) goto out;
    const int64_t limit = (argc == 6) ? (int64_t)sqlite3_value_int64(argv[5]) : -1;      /* -1: none */
    if (argc == 6 && limit < 0) { rc = vtab_error(&vt->base, "%s: limit must not be negative.", fname); goto out; }
    rc = bwithin_radius_arg(vt, fname, argv[3], nq, &radii);
    if (rc != SQLITE_OK) goto out;
    if ((argc == 6 && limit == 0) || nq == 0) goto out;                                  /* no rows, no device (decided here) */
    rc = wmasked_run(c, vt, fname, t, quantized, 1, queries, nq, radii, limit, argv[4]);
out:
    sqlite3_free(owned);
    sqlite3_free(radii);
    return rc;
}

static int full_bwmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bwmasked_filter_common(c, argc, argv, "vector_full_scan_batch_within_filtered", 0); }
static int quant_bwmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bwmasked_filter_common(c, argc, argv, "vector_quantize_scan_batch_within_filtered", 1); }

static sqlite3_module full_bwmasked_module = {0, 0, bwmasked_connect, bwmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_bwmasked_filter,
                                              within_next, within_eof, bwithin_column, bwithin_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_bwmasked_module = {0, 0, bwmasked_connect, bwmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_bwmasked_filter,
                                               within_next, within_eof, bwithin_column, bwithin_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

/* vext_tvf.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * the four table-valued functions of the reference surface: argument checks, scan through the C-ABI
 */
/* ------------------------------------------------------------------------------------------------ table-valued functions */

SCAN_CONNECT(tvf_connect, "CREATE TABLE x(tbl hidden, vector hidden, k hidden, memidx hidden, id, distance);")

static int topk_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return plan_single(info, 1, COL_TBL, COL_MEMIDX); }

static int stream_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 1e8;                   /* no ordering promise (sqlite-vector.c:2245-2275) */
    info->estimatedRows = 100000;
    plan_args(info, COL_TBL, COL_MEMIDX);
    return SQLITE_OK;
}

/* the common xFilter (reference: vCursorFilterCommon, sqlite-vector.c:1723-1826) */
static int filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized, int streaming) {
    static const arg_spec topk_args = {4, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER}}, stream_args = {3, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR}};
    scan_call s;
    scan_begin(&s, cur, fname, quantized, streaming);
    scan_cursor *c = s.c;
    scan_vtab *vt = s.vt;
    int rc = scan_check_args(vt, fname, streaming ? &stream_args : &topk_args, argc, argv);
    if (rc != SQLITE_OK) return rc;
    if ((rc = scan_open(&s, argv, 0, "vector_quantize_scan")) != SQLITE_OK) goto out;     /* (the reference's text names this function whatever was called) */
    table_ctx *t = s.t;
    int k = streaming ? 0 : sqlite3_value_int(argv[3]);
    if (!streaming && k == 0) { rc = SQLITE_DONE; goto out; }       /* sqlite-vector.c:1796 (ends the statement) */
    if (!streaming && k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if ((rc = scan_stage(&s)) != SQLITE_OK) goto out;

    if (streaming) {
        sqlite3_free(c->all_dist); c->all_dist = NULL;
        sqlite3_free(c->all_rowids); c->all_rowids = NULL;
    } else {
        sqlite3_free(c->rowids);
        sqlite3_free(c->distance);
        c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(int64_t));
        c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(double));
        if (!c->rowids || !c->distance) { rc = SQLITE_NOMEM; goto out; }
    }
    int got = 0;
    if (s.ooc) {
        rc = quantized ? ooc_scan_quant(vt->db, t, s.scan_queries, k, c->rowids, c->distance, &got, &c->all_dist, &c->all_rowids, &c->stream_n, &s.err)
                       : ooc_scan_full(vt->db, t, s.scan_queries, k, c->rowids, c->distance, &got, &c->all_dist, &c->all_rowids, &c->stream_n, &s.err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, s.err ? s.err : "scan failed"); goto out; }
        if (!streaming) c->row_count = got;
        goto out;
    }

    scan_lock(&s);
    if (streaming) {
        int64_t n = G.corpus_rows(s.corpus);
        c->all_dist = (float *)sqlite3_malloc64((sqlite3_uint64)(n > 0 ? n : 1) * sizeof(float));
        c->all_rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)(n > 0 ? n : 1) * sizeof(int64_t));
        if (!c->all_dist || !c->all_rowids) { rc = SQLITE_NOMEM; goto out; }
        /* distances AND rowids are copied into the cursor here (the reference's stream cursor reads its own statement,
         * sqlite-vector.c:2277-2313): later re-staging / vector_quantize / cleanup on the table cannot touch them */
        if (n > 0 && (G.scan_distances(s.corpus, t->opt.v_distance, s.scan_queries, c->all_dist) != VG_OK ||
                      G.corpus_rowids(s.corpus, 0, n, c->all_rowids) != VG_OK)) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        c->stream_n = n;
    } else {
        if (G.scan_topk(s.corpus, t->opt.v_distance, s.scan_queries, k, c->rowids, c->distance, &got) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        c->row_count = got;                       /* fewer than k when fewer rows qualify (:1816-1817) */
    }
out:
    return scan_close(&s, rc);
}

static int stream_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return filter_common(cur, argc, argv, fname, quantized, 1); }
static int topk_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return filter_common(cur, argc, argv, fname, quantized, 0); }

SCAN_FORM(scan, "", topk_filter_common, tvf_connect, topk_best_index, tvf_next, tvf_eof, tvf_column, tvf_rowid);
SCAN_FORM(stream, "_stream", stream_filter_common, tvf_connect, stream_best_index, tvf_next, tvf_eof, tvf_column, tvf_rowid);

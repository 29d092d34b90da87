/* vext_topk.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * filtered and paged top-k scans, ordered by (distance, scan position) -
 *     vector_full_scan_filtered / vector_quantize_scan_filtered(table, column, vector, k, filter)                 -> (id, distance)
 *     vector_full_scan_batch_filtered / vector_quantize_scan_batch_filtered(table, column, queries, k, filter)    -> (query, id, distance)
 *     vector_full_scan_after / vector_quantize_scan_after(table, column, vector, k, after_distance, after_rowid)  -> (id, distance)
 *     vector_full_scan_filtered_after / vector_quantize_scan_filtered_after(table, column, vector, k, filter, after_distance, after_rowid)
 * filtered: the k nearest rows among those the filter names.  `filter` is TEXT - ONE read-only SELECT whose first column yields rowids
 * of `table`, prepared on this connection and stepped to the end per call - or a BLOB of packed little-endian int64 rowids.  The
 * question it answers is "... FROM vector_full_scan_stream(...) WHERE id IN (<filter>) ORDER BY distance LIMIT k" without writing,
 * copying and stepping N rows.  The batch form takes the batch functions' `queries` (a BLOB of nq * dim elements or a JSON array of
 * arrays) under ONE filter; each query's rows are what the single form returns for it, and they come by query number (0-based) first.
 * after ("search after"): the next k rows behind a (distance, rowid) cursor - the distance and id of the previous page's last row; both
 * NULL = the first page, exactly one NULL, a cursor that is no number and k outside 1..64 are errors.  A row is behind the cursor when
 * its distance is larger, or equal with a larger rowid: pages never repeat or skip a row, also inside a run of equal distances, and a
 * page taken after the cursor's row was deleted continues where it should.  It answers "... ORDER BY distance, id LIMIT k OFFSET m"
 * without the top-(m + k) scan.
 * Staging, locks, tracked changes and freshness are vector_full_scan's (scan_stage).  The row mask is state of the staged copy, and a
 * copy may be shared by several connections (vext_shared.inc): the mask is set and the scan - of the WHOLE batch - runs inside ONE hold
 * of the lock.  An out-of-core table answers query by query through scan_ooc_query.
 */

SCAN_CONNECT(masked_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, filter hidden);")
SCAN_CONNECT(bmasked_connect, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, k hidden, filter hidden);")
SCAN_CONNECT(after_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, after_distance hidden, after_rowid hidden);")
SCAN_CONNECT(fafter_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, filter hidden, after_distance hidden, after_rowid hidden);")

/* the engine's entry points (masked_set_fn: vext_range.inc) */
typedef int (*masked_scan_fn)(vg_shards *, int, const void *, int, int64_t *, double *, int *);
typedef int (*bmasked_scan_fn)(vg_shards *, int, const void *, int, int, int64_t *, double *, int *);
typedef int (*after_scan_fn)(vg_shards *, int, const void *, int, double, int64_t, int64_t *, double *, int *);

/* the rowids a TEXT filter yields: one statement, read-only, stepped to the end; NULLs and non-integers in its first column are
 * skipped.  Nothing runs when the text is refused. */
static int masked_filter_rowids(scan_vtab *vt, const char *fname, const char *sql, int64_t **out_ids, int64_t *out_n) {
    sqlite3_stmt *st = NULL;
    const char *tail = NULL;
    *out_ids = NULL;
    *out_n = 0;
    if (sqlite3_prepare_v2(vt->db, sql, -1, &st, &tail) != SQLITE_OK)
        return vtab_error(&vt->base, "%s: cannot prepare the filter statement: %s", fname, sqlite3_errmsg(vt->db));
    if (!st) return vtab_error(&vt->base, "%s: the filter holds no statement.", fname);
    while (tail && (*tail == ' ' || *tail == '\t' || *tail == '\n' || *tail == '\r' || *tail == '\f')) ++tail;
    if (tail && *tail) {
        sqlite3_finalize(st);
        return vtab_error(&vt->base, "%s: the filter must be a single statement.", fname);
    }
    /* (BEGIN / COMMIT / ROLLBACK / ATTACH and some PRAGMAs count as read-only and still act on the connection: a statement that yields
     *  no column cannot yield rowids and is refused with them) */
    if (!sqlite3_stmt_readonly(st) || sqlite3_column_count(st) == 0) {
        sqlite3_finalize(st);
        return vtab_error(&vt->base, "%s: the filter must be a read-only statement (a SELECT).", fname);
    }
    int64_t n = 0, cap = 0;
    int64_t *ids = NULL;
    int rc;
    while ((rc = sqlite3_step(st)) == SQLITE_ROW) {
        if (sqlite3_column_type(st, 0) != SQLITE_INTEGER) continue;
        if (n == cap) {
            cap = cap ? cap * 2 : 1024;
            int64_t *grown = (int64_t *)sqlite3_realloc64(ids, (sqlite3_uint64)cap * sizeof(int64_t));
            if (!grown) { sqlite3_free(ids); sqlite3_finalize(st); return SQLITE_NOMEM; }
            ids = grown;
        }
        ids[n++] = (int64_t)sqlite3_column_int64(st, 0);
    }
    if (rc != SQLITE_DONE) {
        rc = vtab_error(&vt->base, "%s: the filter statement failed: %s", fname, sqlite3_errmsg(vt->db));
        sqlite3_finalize(st);
        sqlite3_free(ids);
        return rc;
    }
    sqlite3_finalize(st);
    *out_ids = ids;
    *out_n = n;
    return SQLITE_OK;
}

/* the filter argument of a masked function -> the rowids it names (sqlite3_malloc'd, NULL when it names none): TEXT is one read-only
 * SELECT (masked_filter_rowids), a BLOB holds packed little-endian int64 rowids */
static int masked_filter_arg(scan_vtab *vt, const char *fname, sqlite3_value *arg, int64_t **out_ids, int64_t *out_n) {
    *out_ids = NULL;
    *out_n = 0;
    if (sqlite3_value_type(arg) == SQLITE_TEXT) return masked_filter_rowids(vt, fname, (const char *)sqlite3_value_text(arg), out_ids, out_n);
    const int fbytes = sqlite3_value_bytes(arg);
    if (fbytes % 8) return vtab_error(&vt->base, "%s: a BLOB filter holds packed 64-bit rowids, its length (%d bytes) must be a multiple of 8.", fname, fbytes);
    const int64_t n = fbytes / 8;
    if (n > 0) {                                                                         /* (copied: alignment, and the host's byte order) */
        const uint8_t *p = (const uint8_t *)sqlite3_value_blob(arg);
        int64_t *ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)n * sizeof(int64_t));
        if (!ids) return SQLITE_NOMEM;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t v = 0;
            for (int b = 0; b < 8; ++b) v |= (uint64_t)p[i * 8 + b] << (8 * b);
            ids[i] = (int64_t)v;
        }
        *out_ids = ids;
    }
    *out_n = n;
    return SQLITE_OK;
}

/* One xFilter for the four forms: (table, column, vector | queries, k [, filter] [, after_distance, after_rowid]).  has_filter: the row
 * mask set under the lock.  has_after: a (distance, rowid) cursor - both NULL = the first page. */
static int masked_filter_form(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized, int batch, int has_filter, int has_after) {
    static const arg_spec specs[2][2] = {
        {{5, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_FILTER}}, {7, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_FILTER, ARG_ANY, ARG_ANY}}},
        {{4, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER}}, {6, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_ANY, ARG_ANY}}}};
    const arg_spec *spec = &specs[!has_filter][has_after];
    const int ai = spec->n - 2;
    scan_call s;
    scan_begin(&s, cur, fname, quantized, 0);
    scan_vtab *vt = s.vt;
    int64_t *filter_ids = NULL, filter_n = 0;
    int rc = scan_check_args(vt, fname, spec, argc, argv);
    if (rc != SQLITE_OK) return rc;
    /* the cursor: both NULL = the first page, (-Inf, INT64_MIN) */
    double after_dist = -INFINITY;
    int64_t after_rowid = INT64_MIN;
    if (has_after) {
        const int td = sqlite3_value_type(argv[ai]), tr = sqlite3_value_type(argv[ai + 1]);
        if ((td == SQLITE_NULL) != (tr == SQLITE_NULL))
            return vtab_error(&vt->base, "%s: after_distance and after_rowid must both be NULL (the first page) or both be given.", fname);
        if (td != SQLITE_NULL) {
            if (td != SQLITE_FLOAT && td != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be a number (got %s).", fname, ai + 1, sql_type_name(td));
            if (tr != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, ai + 2, sql_type_name(tr));
            after_dist = sqlite3_value_double(argv[ai]);
            after_rowid = (int64_t)sqlite3_value_int64(argv[ai + 1]);
            if (after_dist != after_dist) return vtab_error(&vt->base, "%s: after_distance cannot be NaN.", fname);
        }
    }
    if ((rc = scan_open(&s, argv, batch, fname)) != SQLITE_OK) goto out;
    table_ctx *t = s.t;
    const int k = sqlite3_value_int(argv[3]);
    if ((k == 0 && !has_after) || s.nq == 0) goto out;                                   /* no rows, no device (decided here) */
    if (k <= 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    /* the allowed rowids: before anything is staged - a refused filter runs nothing */
    if (has_filter && (rc = masked_filter_arg(vt, fname, argv[4], &filter_ids, &filter_n)) != SQLITE_OK) goto out;

    /* an engine without the entry points still loads, the functions then say so */
    const char *const names[3] = {"vg_shards_set_mask_rowids", batch ? "vg_shards_scan_topk_batch_masked" : "vg_shards_scan_topk_masked",
                                  has_filter ? "vg_shards_scan_topk_after_masked" : "vg_shards_scan_topk_after"};
    void *fn[3];
    const char *missing = scan_resolve(&s, names, fn, has_after ? 3 : 2);
    if (missing) {
        rc = batch ? vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked batch scans need a newer libvectorgpu.so).", fname, missing)
                   : vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked scans need a newer libvectorgpu.so).", fname, missing);
        goto out;
    }
    if ((rc = scan_stage(&s)) != SQLITE_OK) goto out;
    if ((rc = scan_topk_buffers(&s, k)) != SQLITE_OK) goto out;

    if (s.ooc) {
        const ooc_keep keep = {NULL, has_filter, filter_ids, filter_n, has_after ? &after_dist : NULL, after_rowid};
        if (filter_n > 1) qsort(filter_ids, (size_t)filter_n, sizeof(int64_t), i64_cmp);
        for (int q = 0; q < s.nq; ++q)                   /* each query reads the table again */
            if ((rc = scan_ooc_topk(&s, q, &keep, k)) != SQLITE_OK) goto out;
    } else {
        int64_t allowed = 0;
        scan_lock(&s);
        if ((has_filter && ((masked_set_fn)fn[0])(s.corpus, filter_ids, filter_n, &allowed) != VG_OK) ||
            (has_after ? ((after_scan_fn)fn[2])(s.corpus, t->opt.v_distance, s.scan_queries, k, after_dist, after_rowid, s.ids, s.dist, s.counts)
             : batch   ? ((bmasked_scan_fn)fn[1])(s.corpus, t->opt.v_distance, s.scan_queries, s.nq, k, s.ids, s.dist, s.counts)
                       : ((masked_scan_fn)fn[1])(s.corpus, t->opt.v_distance, s.scan_queries, k, s.ids, s.dist, s.counts)) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        scan_unlock(&s);
    }
    rc = batch_emit(s.c, s.nq, k, s.ids, s.dist, s.counts);
out:
    sqlite3_free(filter_ids);
    return scan_close(&s, rc);
}

static int masked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return masked_filter_form(cur, argc, argv, fname, quantized, 0, 1, 0); }
static int bmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return masked_filter_form(cur, argc, argv, fname, quantized, 1, 1, 0); }
static int after_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return masked_filter_form(cur, argc, argv, fname, quantized, 0, 0, 1); }
static int fafter_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return masked_filter_form(cur, argc, argv, fname, quantized, 0, 1, 1); }

SCAN_FORM(masked, "_filtered", masked_filter_common, masked_connect, single_best_index, within_next, within_eof, within_column, within_rowid);
SCAN_FORM(bmasked, "_batch_filtered", bmasked_filter_common, bmasked_connect, btopk_best_index, tvf_next, tvf_eof, bmasked_column, tvf_rowid);
SCAN_FORM(after, "_after", after_filter_common, after_connect, single_best_index, within_next, within_eof, within_column, within_rowid);
SCAN_FORM(fafter, "_filtered_after", fafter_filter_common, fafter_connect, single_best_index, within_next, within_eof, within_column, within_rowid);

/* vext_labeled.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * labeled scans, ordered by (distance, scan position) -
 *     vector_full_scan_labeled / vector_quantize_scan_labeled(table, column, vector, k, label_column, label)               -> (id, distance)
 *     vector_full_scan_batch_labeled / vector_quantize_scan_batch_labeled(table, column, queries, k, label_column, labels) -> (query, id, distance)
 * the k nearest rows whose `label_column` equals `label` - the equality filter on a metadata column ("... of this tenant").  The
 * question it answers is "... FROM vector_full_scan_stream(...) JOIN t ... WHERE t.label = ? ORDER BY distance, id LIMIT k" without
 * stepping N rows per call.  The batch form takes the batch functions' `queries` and `labels`, a BLOB of packed little-endian int64, one
 * per query: each query's rows are what the single form returns for it and ITS label, and they come by query number (0-based) first;
 * the engine orders the queries by label and offers a row only to the queries whose label it carries.
 * Label values are SQLite integers in 0 .. 2^32 - 2.  A NULL or non-integer cell is "no label" (the row matches no query); an integer
 * cell outside the range, or such a `label` argument, is an error naming the value.
 * The column is read once - SELECT rowid, "label_column" FROM "table" - mapped to scan positions through the engine's rowid lookup
 * (ascending rowids, as the filter forms need) and set on the staged copy inside the SAME hold of the lock as the scan: a copy may be
 * shared between connections.  Later calls reuse the labels only while the engine still holds labels, they are this
 * connection's labels of that same column on that same handle (a generation on a shared copy says so), and NOTHING has moved since
 * they were read: PRAGMA data_version, sqlite3_total_changes() and the schema version are what they were, and neither the read nor this
 * call sits inside an open transaction.  That is stricter than stage_full's own freshness (an UPDATE of the label column alone moves
 * total_changes; a tracked change or an append behind the staged rows does too) - correct before clever: in doubt the column is read again.
 * An out-of-core table answers query by query through scan_ooc_query against the rowids that carry the query's label (each query reads
 * column and table again): correct, not fast.
 */
#define LABEL_MAX 0xFFFFFFFEll                  /* the largest label; 0xFFFFFFFF is VG_LABEL_NONE */

SCAN_CONNECT(labeled_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, label_column hidden, label hidden);")
SCAN_CONNECT(blabeled_connect, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, k hidden, label_column hidden, labels hidden);")

/* the engine's labeled entry points */
typedef int (*labeled_set_fn)(vg_shards *, const uint32_t *, int64_t);
typedef int (*labeled_has_fn)(const vg_shards *);
typedef int (*labeled_scan_fn)(vg_shards *, int, const void *, int, uint32_t, int64_t *, double *, int *);
typedef int (*blabeled_scan_fn)(vg_shards *, int, const void *, int, const uint32_t *, int, int64_t *, double *, int *);
typedef struct { labeled_set_fn set; labeled_has_fn has; } labeled_api;

/* a label given as an argument (or an element of the batch's BLOB): in range, or an error naming the value */
static int labeled_label_value(scan_vtab *vt, const char *fname, int64_t v, uint32_t *out) {
    if (v < 0 || v > LABEL_MAX) return vtab_error(&vt->base, "%s: label %lld is out of range (labels are integers in 0 .. 4294967294).", fname, (long long)v);
    *out = (uint32_t)v;
    return SQLITE_OK;
}

/* "name" with embedded quotes doubled */
static char *labeled_quoted(const char *name) { return sqlite3_mprintf("\"%w\"", name); }

static uint64_t g_label_gen;                    /* generations handed to shared copies (atomic) */

/* One pass over SELECT rowid, "label_column" FROM "table".  corpus != NULL: labels[n_rows] by scan position (VG_LABEL_NONE where the
 * row has none, or is not staged).  corpus == NULL (out of core): the rowids whose label is `want`, for the slab route.  An integer cell
 * out of range is an error naming the value. */
static int labeled_read_column(scan_vtab *vt, const char *fname, table_ctx *t, const char *label_col, vg_shards *corpus, uint32_t *labels,
                               int64_t n_rows, uint32_t want, int64_t **out_ids, int64_t *out_n) {
    char *qt = labeled_quoted(t->t_name), *qc = labeled_quoted(label_col);
    char *sql = (qt && qc) ? sqlite3_mprintf("SELECT rowid, %s FROM %s;", qc, qt) : NULL;
    sqlite3_free(qt);
    sqlite3_free(qc);
    if (!sql) return SQLITE_NOMEM;
    sqlite3_stmt *st = NULL;
    int rc = sqlite3_prepare_v2(vt->db, sql, -1, &st, NULL);
    sqlite3_free(sql);
    if (rc != SQLITE_OK) return vtab_error(&vt->base, "%s: cannot read label column '%s' of table '%s': %s", fname, label_col, t->t_name, sqlite3_errmsg(vt->db));
    int64_t n = 0, cap = 0, *ids = NULL;
    while ((rc = sqlite3_step(st)) == SQLITE_ROW) {
        if (sqlite3_column_type(st, 1) != SQLITE_INTEGER) continue;                      /* NULL / non-integer: no label */
        const int64_t rowid = (int64_t)sqlite3_column_int64(st, 0), v = (int64_t)sqlite3_column_int64(st, 1);
        if (v < 0 || v > LABEL_MAX) {
            rc = vtab_error(&vt->base, "%s: label %lld of rowid %lld in column '%s' is out of range (labels are integers in 0 .. 4294967294).",
                            fname, (long long)v, (long long)rowid, label_col);
            goto fail;
        }
        if (corpus) {
            const int64_t p = G.corpus_find_rowid(corpus, rowid);
            if (p == -2) { rc = vtab_error(&vt->base, "%s: the staged rowids are not ascending (no rowid lookup).", fname); goto fail; }
            if (p >= 0 && p < n_rows) labels[p] = (uint32_t)v;                         /* (a row that is not staged - a NULL vector - has no position) */
        } else if ((uint32_t)v == want) {
            if (n == cap) {
                cap = cap ? cap * 2 : 1024;
                int64_t *grown = (int64_t *)sqlite3_realloc64(ids, (sqlite3_uint64)cap * sizeof(int64_t));
                if (!grown) { rc = SQLITE_NOMEM; goto fail; }
                ids = grown;
            }
            ids[n++] = rowid;
        }
    }
    if (rc != SQLITE_DONE) { rc = vtab_error(&vt->base, "%s: reading label column '%s' failed: %s", fname, label_col, sqlite3_errmsg(vt->db)); goto fail; }
    sqlite3_finalize(st);
    if (out_ids) { *out_ids = ids; *out_n = n; } else sqlite3_free(ids);
    return SQLITE_OK;
fail:
    sqlite3_finalize(st);
    sqlite3_free(ids);
    return rc;
}

/* the rowids of an out-of-core table whose label is `want`, sorted: what scan_ooc_query filters against */
static int labeled_rowids_of(scan_vtab *vt, const char *fname, table_ctx *t, const char *label_col, uint32_t want, int64_t **out_ids, int64_t *out_n) {
    *out_ids = NULL; *out_n = 0;
    int rc = labeled_read_column(vt, fname, t, label_col, NULL, NULL, 0, want, out_ids, out_n);
    if (rc == SQLITE_OK && *out_n > 1) qsort(*out_ids, (size_t)*out_n, sizeof(int64_t), i64_cmp);
    return rc;
}

/* Called INSIDE the hold of full_lock / quant_lock: the staged copy carries this connection's labels of `label_col` when it returns
 * SQLITE_OK - reused when nothing has moved since they were read (the file's head comment has the rule), read and set otherwise. */
static int labeled_ensure(scan_vtab *vt, const char *fname, table_ctx *t, int quantized, vg_shards *corpus, const labeled_api *api, const char *label_col) {
    const int q = quantized ? 1 : 0;
    shared_corpus *sh = quantized ? t->quant_sh : t->full_sh;
    int64_t dv, ch, sv;
    db_stamps(vt->db, &dv, &ch, &sv);
    const int in_txn = !sqlite3_get_autocommit(vt->db);
    if (t->lab_col[q] && !strcmp(t->lab_col[q], label_col) && t->lab_corpus[q] == corpus && !t->lab_in_txn[q] && !in_txn &&
        t->lab_data_version[q] == dv && t->lab_changes[q] == ch && t->lab_schema[q] == sv &&
        (!sh || sh->label_gen == t->lab_gen[q]) && api->has(corpus))
        return SQLITE_OK;
    sqlite3_free(t->lab_col[q]);                                                       /* (whatever happens below: no claim on the old labels) */
    t->lab_col[q] = NULL;
    const int64_t n_rows = G.corpus_rows(corpus);
    uint32_t *labels = (uint32_t *)sqlite3_malloc64((sqlite3_uint64)(n_rows > 0 ? n_rows : 1) * sizeof(uint32_t));
    if (!labels) return SQLITE_NOMEM;
    for (int64_t i = 0; i < n_rows; ++i) labels[i] = VG_LABEL_NONE;
    int rc = labeled_read_column(vt, fname, t, label_col, corpus, labels, n_rows, 0, NULL, NULL);
    if (rc == SQLITE_OK && api->set(corpus, labels, n_rows) != VG_OK) rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
    sqlite3_free(labels);
    if (rc != SQLITE_OK) return rc;
    t->lab_col[q] = dup_str(label_col);                                                /* (no memory: the next call reads again) */
    t->lab_corpus[q] = corpus;
    t->lab_data_version[q] = dv; t->lab_changes[q] = ch; t->lab_schema[q] = sv; t->lab_in_txn[q] = in_txn;
    t->lab_gen[q] = __atomic_add_fetch(&g_label_gen, 1, __ATOMIC_RELAXED);
    if (sh) sh->label_gen = t->lab_gen[q];
    return SQLITE_OK;
}

/* One xFilter for both forms: (table, column, vector | queries, k, label_column, label | labels) */
static int labeled_filter_form(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized, int batch) {
    static const arg_spec specs[2] = {{6, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_TEXT, ARG_INTEGER}},
                                      {6, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_TEXT, ARG_ANY}}};
    scan_call s;
    scan_begin(&s, cur, fname, quantized, 0);
    scan_vtab *vt = s.vt;
    uint32_t *qlabels = NULL, label = 0;
    int rc = scan_check_args(vt, fname, &specs[batch], argc, argv);
    if (rc != SQLITE_OK) return rc;
    if (batch && sqlite3_value_type(argv[5]) != SQLITE_BLOB)
        return vtab_error(&vt->base, "%s: argument %d must be a BLOB of packed 64-bit labels (got %s).", fname, 6, sql_type_name(sqlite3_value_type(argv[5])));
    const char *label_col = (const char *)sqlite3_value_text(argv[4]);
    if ((rc = scan_lookup(&s, argv)) != SQLITE_OK) goto out;
    table_ctx *t = s.t;
    /* (the single form's label is checked before its query is decoded) */
    if (!batch && (rc = labeled_label_value(vt, fname, (int64_t)sqlite3_value_int64(argv[5]), &label)) != SQLITE_OK) goto out;
    if ((rc = scan_open(&s, argv, batch, fname)) != SQLITE_OK) goto out;
    if (batch) {
        /* one label per query (copied: alignment, and the host's byte order), each checked before anything is staged */
        const int lbytes = sqlite3_value_bytes(argv[5]);
        const uint8_t *p = (const uint8_t *)sqlite3_value_blob(argv[5]);
        if (lbytes % 8 || lbytes / 8 != s.nq) {
            rc = vtab_error(&vt->base, "%s: the labels hold %d bytes, expected %d (one packed 64-bit label per query, %d queries).", fname, lbytes, s.nq * 8, s.nq);
            goto out;
        }
        qlabels = (uint32_t *)sqlite3_malloc64((sqlite3_uint64)(s.nq > 0 ? s.nq : 1) * sizeof(uint32_t));
        if (!qlabels) { rc = SQLITE_NOMEM; goto out; }
        for (int i = 0; i < s.nq; ++i) {
            uint64_t v = 0;
            for (int b = 0; b < 8; ++b) v |= (uint64_t)p[i * 8 + b] << (8 * b);
            if ((rc = labeled_label_value(vt, fname, (int64_t)v, &qlabels[i])) != SQLITE_OK) goto out;
        }
    }
    const uint32_t *labels = batch ? qlabels : &label;
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0 || s.nq == 0) goto out;                                                   /* no rows, no device (decided here) */
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    /* an engine without the entry points still loads, the functions then say so */
    const char *const names[3] = {"vg_shards_set_labels", "vg_shards_has_labels", batch ? "vg_shards_scan_topk_batch_labeled" : "vg_shards_scan_topk_labeled"};
    void *fn[3];
    const char *missing = scan_resolve(&s, names, fn, 3);
    if (missing) {
        rc = batch ? vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (labeled batch scans need a newer libvectorgpu.so).", fname, missing)
                   : vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (labeled scans need a newer libvectorgpu.so).", fname, missing);
        goto out;
    }
    const labeled_api api = {(labeled_set_fn)fn[0], (labeled_has_fn)fn[1]};
    if ((rc = scan_stage(&s)) != SQLITE_OK) goto out;
    if ((rc = scan_topk_buffers(&s, k)) != SQLITE_OK) goto out;

    if (s.ooc) {
        for (int q = 0; q < s.nq; ++q) {
            ooc_keep keep = {NULL, 1, NULL, 0, NULL, 0};
            int64_t *lab_ids = NULL;
            rc = labeled_rowids_of(vt, fname, t, label_col, labels[q], &lab_ids, &keep.n_ids);
            keep.ids = lab_ids;
            if (rc == SQLITE_OK) rc = scan_ooc_topk(&s, q, &keep, k);
            sqlite3_free(lab_ids);
            if (rc != SQLITE_OK) goto out;
        }
    } else {
        /* the labels are state of the staged copy, which other connections may hold too: make sure of them and scan inside one hold of the lock */
        scan_lock(&s);
        if ((rc = labeled_ensure(vt, fname, t, quantized, s.corpus, &api, label_col)) != SQLITE_OK) goto out;
        if ((batch ? ((blabeled_scan_fn)fn[2])(s.corpus, t->opt.v_distance, s.scan_queries, s.nq, labels, k, s.ids, s.dist, s.counts)
                   : ((labeled_scan_fn)fn[2])(s.corpus, t->opt.v_distance, s.scan_queries, k, labels[0], s.ids, s.dist, s.counts)) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        scan_unlock(&s);
    }
    rc = batch_emit(s.c, s.nq, k, s.ids, s.dist, s.counts);
out:
    sqlite3_free(qlabels);
    return scan_close(&s, rc);
}

static int labeled_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return labeled_filter_form(cur, argc, argv, fname, quantized, 0); }
static int blabeled_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return labeled_filter_form(cur, argc, argv, fname, quantized, 1); }

SCAN_FORM(labeled, "_labeled", labeled_filter_common, labeled_connect, single_best_index, within_next, within_eof, within_column, within_rowid);
SCAN_FORM(blabeled, "_batch_labeled", blabeled_filter_common, blabeled_connect, btopk_best_index, tvf_next, tvf_eof, bmasked_column, tvf_rowid);

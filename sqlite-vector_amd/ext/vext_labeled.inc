/* vext_labeled.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * labeled scans: vector_full_scan_labeled / vector_quantize_scan_labeled(table, column, vector, k, label_column, label) -> (id, distance),
 * the k nearest rows whose `label_column` equals `label`, ordered by (distance, scan position) - the equality filter on a metadata
 * column ("... of this tenant").  The question it answers is "... FROM vector_full_scan_stream(...) JOIN t ... WHERE t.label = ? ORDER
 * BY distance, id LIMIT k" without stepping N rows per call.
 * Label values are SQLite integers in 0 .. 2^32 - 2.  A NULL or non-integer cell is "no label" (the row matches no query); an integer
 * cell outside the range, or such a `label` argument, is an error naming the value.
 * The column is read once - SELECT rowid, "label_column" FROM "table" - mapped to scan positions through the engine's rowid lookup
 * (ascending rowids, as the filter forms need) and set on the staged copy inside the SAME hold of full_lock / quant_lock as the scan: a
 * copy may be shared between connections.  Later calls reuse the labels only while the engine still holds labels, they are this
 * connection's labels of that same column on that same handle (a generation on a shared copy says so), and NOTHING has moved since
 * they were read: PRAGMA data_version, sqlite3_total_changes() and the schema version are what they were, and neither the read nor this
 * call sits inside an open transaction.  That is stricter than stage_full's own freshness (an UPDATE of the label column alone moves
 * total_changes; a tracked change or an append behind the staged rows does too) - correct before clever: in doubt the column is read again.
 * An out-of-core table answers through the slab path with k = 0, a host-side label compare and a sort: correct, not fast.
 * Staging, cursor, columns and index plan are the filtered functions' (vext_masked.inc, vext_within.inc).  labeled_label_value,
 * labeled_resolve, labeled_ensure and labeled_rowids_of are shared with the batch form (vext_batch_labeled.inc).
 */
#define LABEL_MAX 0xFFFFFFFEll                  /* the largest label; 0xFFFFFFFF is VG_LABEL_NONE */

enum { LCOL_TBL = 2, LCOL_LABEL = 7 };

static int labeled_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, label_column hidden, label hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int labeled_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 1.0;
    info->estimatedRows = 100;
    info->orderByConsumed = 1;                   /* output is distance-ascending, like the top-k functions */
    info->idxNum = 1;
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ) continue;
        if (c->iColumn >= LCOL_TBL && c->iColumn <= LCOL_LABEL) {
            info->aConstraintUsage[i].argvIndex = c->iColumn - LCOL_TBL + 1;
            info->aConstraintUsage[i].omit = 1;
        }
    }
    return SQLITE_OK;
}

/* the engine's labeled entry points, resolved like the masked ones: an engine without them still loads, the functions then say so */
typedef int (*labeled_set_fn)(vg_shards *, const uint32_t *, int64_t);
typedef int (*labeled_has_fn)(const vg_shards *);
typedef int (*labeled_scan_fn)(vg_shards *, int, const void *, int, uint32_t, int64_t *, double *, int *);
typedef int (*blabeled_scan_fn)(vg_shards *, int, const void *, int, const uint32_t *, int, int64_t *, double *, int *);
typedef struct { labeled_set_fn set; labeled_has_fn has; labeled_scan_fn scan; blabeled_scan_fn scan_batch; } labeled_api;
static const char *labeled_resolve(labeled_api *a, int batch) {
    memset(a, 0, sizeof(*a));
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    a->set = (labeled_set_fn)dlsym(G.handle, "vg_shards_set_labels");
    if (!a->set) return "vg_shards_set_labels";
    a->has = (labeled_has_fn)dlsym(G.handle, "vg_shards_has_labels");
    if (!a->has) return "vg_shards_has_labels";
    if (batch) {
        a->scan_batch = (blabeled_scan_fn)dlsym(G.handle, "vg_shards_scan_topk_batch_labeled");
        if (!a->scan_batch) return "vg_shards_scan_topk_batch_labeled";
    } else {
        a->scan = (labeled_scan_fn)dlsym(G.handle, "vg_shards_scan_topk_labeled");
        if (!a->scan) return "vg_shards_scan_topk_labeled";
    }
    return NULL;
}

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

/* the rowids of an out-of-core table whose label is `want`, sorted: what masked_ooc_topk filters against */
static int labeled_rowids_of(scan_vtab *vt, const char *fname, table_ctx *t, const char *label_col, uint32_t want, int64_t **out_ids, int64_t *out_n) {
    *out_ids = NULL; *out_n = 0;
    int rc = labeled_read_column(vt, fname, t, label_col, NULL, NULL, 0, want, out_ids, out_n);
    if (rc == SQLITE_OK && *out_n > 1) qsort(*out_ids, (size_t)*out_n, sizeof(int64_t), masked_i64_cmp);
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

static int labeled_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->stream_pos = 0;
    c->stream_n = 0;
    if (argc != 6) return vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, 6, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if ((i < 2 || i == 4) && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 2 && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if ((i == 3 || i == 5) && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
    const char *label_col = (const char *)sqlite3_value_text(argv[4]);
    table_ctx *t = context_lookup(vt->ctx, tbl, col);
    if (!t) return vtab_error(&vt->base, "%s: unable to retrieve context.", fname);
    uint32_t label = 0;
    int rc = labeled_label_value(vt, fname, (int64_t)sqlite3_value_int64(argv[5]), &label);
    if (rc != SQLITE_OK) return rc;

    const void *query = NULL;
    void *owned = NULL;
    int qbytes = 0;
    if (sqlite3_value_type(argv[2]) == SQLITE_TEXT) {
        owned = vector_from_json(NULL, &vt->base, t->opt.v_type, (const char *)sqlite3_value_text(argv[2]), &qbytes, t->opt.v_dim);
        if (!owned) return SQLITE_ERROR;
        query = owned;
    } else {
        query = sqlite3_value_blob(argv[2]);
        qbytes = sqlite3_value_bytes(argv[2]);
        if (!query) return vtab_error(&vt->base, "%s: input vector cannot be NULL.", fname);
    }
    char *err = NULL;
    uint8_t *qquant = NULL;
    int64_t *ooc_ids = NULL;
    if (qbytes < t->opt.v_dim * elem_size(t->opt.v_type)) {
        rc = vtab_error(&vt->base, "%s: query vector has %d bytes, expected %d.", fname, qbytes, t->opt.v_dim * elem_size(t->opt.v_type));
        goto out;
    }
    if (quantized) {
        char name[SQL_BUF];
        sqlite3_snprintf(sizeof(name), name, "vector0_%q_%q", tbl, col);
        if (!exists_in_master(vt->db, "table", name)) {
            rc = vtab_error(&vt->base, "Quantization table not found for table '%s' and column '%s'. Ensure that vector_quantize() has been called before using %s().", tbl, col, fname);
            goto out;
        }
    }
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0) goto out;                                                                /* no rows, no device (decided here) */
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    labeled_api api;
    const char *missing = labeled_resolve(&api, 0);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (labeled scans need a newer libvectorgpu.so).", fname, missing); goto out; }

    vg_shards *corpus = NULL;
    const void *scan_query = query;
    if (quantized) {
        if (!t->quant_preloaded || !t->quant) rc = stage_quant(vt->db, t, 0, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        qquant = (uint8_t *)sqlite3_malloc(t->opt.v_dim);
        if (!qquant) { rc = SQLITE_NOMEM; goto out; }
        if (G.quantize_query(t->opt.v_type, query, t->opt.v_dim, t->scale, t->offset, t->opt.q_type, qquant) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        scan_query = qquant;
        corpus = t->quant;
    } else {
        rc = stage_full(vt->db, vt->ctx, t, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        corpus = t->full;
    }
    if (!api.scan) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(int64_t));
    c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(double));
    if (!c->rowids || !c->distance) { rc = SQLITE_NOMEM; goto out; }

    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: the rowids of the label from the column, then every distance through the slab path
         * (k = 0), compared, sorted and cut on the host */
        int64_t held = 0, n_ids = 0;
        rc = labeled_rowids_of(vt, fname, t, label_col, label, &ooc_ids, &n_ids);
        if (rc == SQLITE_OK) rc = masked_ooc_topk(vt, fname, t, quantized, scan_query, k, ooc_ids, n_ids, c->rowids, c->distance, &held);
        if (rc == SQLITE_OK) c->stream_n = held;
        goto out;
    }

    /* the labels are state of the staged copy, which other connections may hold too: make sure of them and scan inside one hold of the lock */
    if (quantized) quant_lock(t); else full_lock(t);
    {
        int got = 0;
        rc = labeled_ensure(vt, fname, t, quantized, corpus, &api, label_col);
        if (rc == SQLITE_OK && api.scan(corpus, t->opt.v_distance, scan_query, k, label, c->rowids, c->distance, &got) != VG_OK)
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
        if (rc == SQLITE_OK) c->stream_n = got;
    }
    if (quantized) quant_unlock(t); else full_unlock(t);
out:
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(ooc_ids);
    return rc;
}

static int full_labeled_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return labeled_filter_common(c, argc, argv, "vector_full_scan_labeled", 0); }
static int quant_labeled_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return labeled_filter_common(c, argc, argv, "vector_quantize_scan_labeled", 1); }

static sqlite3_module full_labeled_module = {0, 0, labeled_connect, labeled_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_labeled_filter,
                                             within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_labeled_module = {0, 0, labeled_connect, labeled_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_labeled_filter,
                                              within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

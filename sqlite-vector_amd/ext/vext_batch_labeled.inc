/* vext_batch_labeled.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * labeled batch scans: vector_full_scan_batch_labeled / vector_quantize_scan_batch_labeled(table, column, queries, k, label_column,
 * labels) -> (query, id, distance): for every query of the batch the k nearest rows whose `label_column` equals THAT query's label,
 * ordered by query number (0-based), then (distance, scan position).  `queries` is the batch functions' argument (vext_batch.inc),
 * `labels` a BLOB of packed little-endian int64, one per query, each in 0 .. 2^32 - 2.  Each query's rows are what
 * vector_full_scan_labeled returns for it and its label.
 * Label column, reuse rule, lock and engine entry points are the single form's (vext_labeled.inc); the engine orders the queries by
 * label and offers a row only to the queries whose label it carries (vg_shards_scan_topk_batch_labeled).  An out-of-core table answers
 * query by query through the single form's slab route: correct, not fast.  Cursor, columns and index plan are the masked batch's
 * (vext_batch_masked.inc), with one more hidden column.
 */
enum { BLCOL_QUERY = 0, BLCOL_DISTANCE = 2, BLCOL_TBL = 3, BLCOL_LABELS = 8 };

static int blabeled_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, k hidden, label_column hidden, labels hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int blabeled_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 10.0;
    info->estimatedRows = 1000;
    info->idxNum = 3;
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ) continue;
        if (c->iColumn >= BLCOL_TBL && c->iColumn <= BLCOL_LABELS) {
            info->aConstraintUsage[i].argvIndex = c->iColumn - BLCOL_TBL + 1;
            info->aConstraintUsage[i].omit = 1;
        }
    }
    /* rows come out as (query asc, distance asc): claim the order only when that is what was asked for */
    if (info->nOrderBy == 2 && info->aOrderBy[0].iColumn == BLCOL_QUERY && !info->aOrderBy[0].desc &&
        info->aOrderBy[1].iColumn == BLCOL_DISTANCE && !info->aOrderBy[1].desc) info->orderByConsumed = 1;
    if (info->nOrderBy == 1 && info->aOrderBy[0].iColumn == BLCOL_QUERY && !info->aOrderBy[0].desc) info->orderByConsumed = 1;
    return SQLITE_OK;
}

static int blabeled_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->row_index = 0;
    c->row_count = 0;
    if (argc != 6) return vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, 6, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if ((i < 2 || i == 4) && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 2 && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 5 && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be a BLOB of packed 64-bit labels (got %s).", fname, i + 1, sql_type_name(t));
    }
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
    const char *label_col = (const char *)sqlite3_value_text(argv[4]);
    table_ctx *t = context_lookup(vt->ctx, tbl, col);
    if (!t) return vtab_error(&vt->base, "%s: unable to retrieve context.", fname);
    const int dim = t->opt.v_dim;
    const int64_t qrow = (int64_t)dim * elem_size(t->opt.v_type);

    const uint8_t *queries = NULL;
    void *owned = NULL;
    uint8_t *qquant = NULL;
    int64_t *ids = NULL;
    double *dist = NULL;
    int *counts = NULL;
    uint32_t *qlabels = NULL;
    char *err = NULL;
    int nq = 0;
    int rc = batch_queries_arg(vt, fname, t, argv[2], &queries, &owned, &nq);
    if (rc != SQLITE_OK) return rc;
    if (quantized) {
        char name[SQL_BUF];
        sqlite3_snprintf(sizeof(name), name, "vector0_%q_%q", tbl, col);
        if (!exists_in_master(vt->db, "table", name)) {
            rc = vtab_error(&vt->base, "Quantization table not found for table '%s' and column '%s'. Ensure that vector_quantize() has been called before using %s().", tbl, col, fname);
            goto out;
        }
    }
    /* one label per query (copied: alignment, and the host's byte order), each checked before anything is staged */
    {
        const int lbytes = sqlite3_value_bytes(argv[5]);
        const uint8_t *p = (const uint8_t *)sqlite3_value_blob(argv[5]);
        if (lbytes % 8 || lbytes / 8 != nq) {
            rc = vtab_error(&vt->base, "%s: the labels hold %d bytes, expected %d (one packed 64-bit label per query, %d queries).", fname, lbytes, nq * 8, nq);
            goto out;
        }
        qlabels = (uint32_t *)sqlite3_malloc64((sqlite3_uint64)(nq > 0 ? nq : 1) * sizeof(uint32_t));
        if (!qlabels) { rc = SQLITE_NOMEM; goto out; }
        for (int i = 0; i < nq; ++i) {
            uint64_t v = 0;
            for (int b = 0; b < 8; ++b) v |= (uint64_t)p[i * 8 + b] << (8 * b);
            rc = labeled_label_value(vt, fname, (int64_t)v, &qlabels[i]);
            if (rc != SQLITE_OK) goto out;
        }
    }
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0 || nq == 0) goto out;                                                     /* no rows, no device (decided here) */
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    labeled_api api;
    const char *missing = labeled_resolve(&api, 1);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (labeled batch scans need a newer libvectorgpu.so).", fname, missing); goto out; }

    vg_shards *corpus = NULL;
    const void *scan_queries = queries;
    int64_t qstep = qrow;
    if (quantized) {
        if (!t->quant_preloaded || !t->quant) rc = stage_quant(vt->db, t, 0, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        rc = batch_quantize_queries(vt, fname, t, queries, nq, &qquant);
        if (rc != SQLITE_OK) goto out;
        scan_queries = qquant;
        qstep = dim;
        corpus = t->quant;
    } else {
        rc = stage_full(vt->db, vt->ctx, t, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        corpus = t->full;
    }
    if (!api.scan_batch) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * k * sizeof(int64_t));
    dist = (double *)sqlite3_malloc64((sqlite3_uint64)nq * k * sizeof(double));
    counts = (int *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int));
    if (!ids || !dist || !counts) { rc = SQLITE_NOMEM; goto out; }
    memset(counts, 0, (size_t)nq * sizeof(int));

    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: query by query through the single form's route - each query reads column and table again */
        for (int i = 0; i < nq; ++i) {
            int64_t held = 0, n_ids = 0, *lab_ids = NULL;
            rc = labeled_rowids_of(vt, fname, t, label_col, qlabels[i], &lab_ids, &n_ids);
            if (rc == SQLITE_OK)
                rc = masked_ooc_topk(vt, fname, t, quantized, (const uint8_t *)scan_queries + i * qstep, k, lab_ids, n_ids,
                                     ids + (int64_t)i * k, dist + (int64_t)i * k, &held);
            sqlite3_free(lab_ids);
            if (rc != SQLITE_OK) goto out;
            counts[i] = (int)held;
        }
    } else {
        /* the labels are state of the staged copy, which other connections may hold too: make sure of them and scan the batch inside one hold of the lock */
        if (quantized) quant_lock(t); else full_lock(t);
        rc = labeled_ensure(vt, fname, t, quantized, corpus, &api, label_col);
        if (rc == SQLITE_OK && api.scan_batch(corpus, t->opt.v_distance, scan_queries, nq, qlabels, k, ids, dist, counts) != VG_OK)
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
        if (quantized) quant_unlock(t); else full_unlock(t);
        if (rc != SQLITE_OK) goto out;
    }
    rc = batch_emit(c, nq, k, ids, dist, counts);
out:
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(ids);
    sqlite3_free(dist);
    sqlite3_free(counts);
    sqlite3_free(qlabels);
    return rc;
}

static int full_blabeled_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return blabeled_filter_common(c, argc, argv, "vector_full_scan_batch_labeled", 0); }
static int quant_blabeled_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return blabeled_filter_common(c, argc, argv, "vector_quantize_scan_batch_labeled", 1); }

static sqlite3_module full_blabeled_module = {0, 0, blabeled_connect, blabeled_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_blabeled_filter,
                                              tvf_next, tvf_eof, bmasked_column, tvf_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_blabeled_module = {0, 0, blabeled_connect, blabeled_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_blabeled_filter,
                                               tvf_next, tvf_eof, bmasked_column, tvf_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

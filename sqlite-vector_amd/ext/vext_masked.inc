/* vext_masked.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * masked scans: vector_full_scan_filtered / vector_quantize_scan_filtered(table, column, vector, k, filter) -> (id, distance), the k
 * nearest rows among those the filter names, ordered by (distance, scan position).  `filter` is TEXT - ONE read-only SELECT whose
 * first column yields rowids of `table`, prepared on this connection and stepped to the end per call - or a BLOB of packed
 * little-endian int64 rowids.  The question it answers is "... FROM vector_full_scan_stream(...) WHERE id IN (<filter>) ORDER BY
 * distance LIMIT k" without writing, copying and stepping N rows.
 * Staging, locks, tracked changes and freshness are vector_full_scan's (stage_full / stage_quant).  The row mask is state of the
 * staged copy, and a copy may be shared by several connections (vext_shared.inc): the mask is set and the scan runs inside ONE hold
 * of full_lock / quant_lock.  An out-of-core table answers through the slab path with k = 0 and a filter + sort here: correct, not
 * fast (INTEGRATION.md).  Cursor, columns and index plan are the within functions' (vext_within.inc).  The filter argument and the
 * out-of-core answer are helpers (masked_filter_arg, masked_ooc_topk) shared with the batch form (vext_batch_masked.inc).
 */
static int masked_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, filter hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

/* the engine's masked-scan entry points, resolved like the range scans': an engine without them still loads, the functions then say so */
typedef int (*masked_set_fn)(vg_shards *, const int64_t *, int64_t, int64_t *);
typedef int (*masked_scan_fn)(vg_shards *, int, const void *, int, int64_t *, double *, int *);
static const char *masked_resolve(masked_set_fn *set, masked_scan_fn *scan) {
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    *set = (masked_set_fn)dlsym(G.handle, "vg_shards_set_mask_rowids");
    if (!*set) return "vg_shards_set_mask_rowids";
    *scan = (masked_scan_fn)dlsym(G.handle, "vg_shards_scan_topk_masked");
    if (!*scan) return "vg_shards_scan_topk_masked";
    return NULL;
}

static int masked_i64_cmp(const void *a, const void *b) {
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return (x > y) - (x < y);
}

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

/* one query against a table that does not fit the device: every distance through the slab path (k = 0), filtered against the SORTED
 * rowids, sorted by (distance, scan position) and cut to k here; out_ids / out_dist hold k slots */
/* (has_filter = 0: every row is allowed; after_dist != NULL: only rows behind the cursor (*after_dist, after_rowid) of the paged forms,
 * vext_after.inc - (double)d > D, or d == D and rowid > R) */
static int masked_ooc_topk_ex(scan_vtab *vt, const char *fname, table_ctx *t, int quantized, const void *scan_query, int k, int has_filter,
                              const int64_t *sorted_ids, int64_t filter_n, const double *after_dist, int64_t after_rowid,
                              int64_t *out_ids, double *out_dist, int64_t *out_held) {
    char *err = NULL;
    float *all_dist = NULL;
    int64_t *all_ids = NULL;
    int got = 0;
    int64_t n = 0;
    *out_held = 0;
    int rc = quantized ? ooc_scan_quant(vt->db, t, scan_query, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err)
                       : ooc_scan_full(vt->db, t, scan_query, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err);
    if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "scan failed"); goto done; }
    within_hit *hits = (within_hit *)sqlite3_malloc64((sqlite3_uint64)(n > 0 ? n : 1) * sizeof(within_hit));
    if (!hits) { rc = SQLITE_NOMEM; goto done; }
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!(all_dist[i] < INFINITY) || (has_filter && filter_n == 0)) continue;        /* NaN / +Inf never enter */
        if (has_filter && !bsearch(&all_ids[i], sorted_ids, (size_t)filter_n, sizeof(int64_t), masked_i64_cmp)) continue;
        if (after_dist && !((double)all_dist[i] > *after_dist || ((double)all_dist[i] == *after_dist && all_ids[i] > after_rowid))) continue;
        hits[m].d = all_dist[i]; hits[m].pos = i; ++m;
    }
    qsort(hits, (size_t)m, sizeof(within_hit), within_hit_cmp);
    const int64_t held = (m < k) ? m : k;
    for (int64_t i = 0; i < held; ++i) { out_ids[i] = all_ids[hits[i].pos]; out_dist[i] = (double)hits[i].d; }
    sqlite3_free(hits);
    *out_held = held;
done:
    sqlite3_free(err);
    sqlite3_free(all_dist);
    sqlite3_free(all_ids);
    return rc;
}

static int masked_ooc_topk(scan_vtab *vt, const char *fname, table_ctx *t, int quantized, const void *scan_query, int k,
                           const int64_t *sorted_ids, int64_t filter_n, int64_t *out_ids, double *out_dist, int64_t *out_held) {
    return masked_ooc_topk_ex(vt, fname, t, quantized, scan_query, k, 1, sorted_ids, filter_n, NULL, 0, out_ids, out_dist, out_held);
}

/* the paged forms' entry points (vext_after.inc), resolved like the masked ones */
typedef int (*after_scan_fn)(vg_shards *, int, const void *, int, double, int64_t, int64_t *, double *, int *);

/* One filter routine for the masked scans and the paged scans (vext_after.inc), which differ in their argument list and the engine
 * call only: (table, column, vector, k [, filter] [, after_distance, after_rowid]).  has_filter: a filter argument, the row mask set
 * under the lock.  has_after: a (distance, rowid) cursor - both NULL = the first page. */
static int masked_filter_form(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized, int has_filter, int has_after) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->stream_pos = 0;
    c->stream_n = 0;
    const int want_argc = 4 + (has_filter ? 1 : 0) + (has_after ? 2 : 0), fi = has_filter ? 4 : -1, ai = has_after ? want_argc - 2 : -1;
    if (argc != want_argc) return vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, want_argc, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if (i < 2 && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == fi && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: filter cannot be NULL.", fname);
        if ((i == 2 || i == fi) && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
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
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
    table_ctx *t = context_lookup(vt->ctx, tbl, col);
    if (!t) return vtab_error(&vt->base, "%s: unable to retrieve context.", fname);

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
    int rc = SQLITE_OK;
    char *err = NULL;
    uint8_t *qquant = NULL;
    int64_t *filter_owned = NULL;
    const int64_t *filter_ids = NULL;
    int64_t filter_n = 0;
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
    if (k == 0 && !has_after) goto out;                                                  /* no rows, no device (decided here) */
    if (k <= 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    /* the allowed rowids: before anything is staged - a refused filter runs nothing */
    if (has_filter) rc = masked_filter_arg(vt, fname, argv[4], &filter_owned, &filter_n);
    if (rc != SQLITE_OK) goto out;
    filter_ids = filter_owned;

    masked_set_fn set_mask = NULL;
    masked_scan_fn scan = NULL;
    after_scan_fn scan_after = NULL;
    const char *missing = masked_resolve(&set_mask, &scan);
    if (!missing && has_after && G.handle) {
        const char *sym = has_filter ? "vg_shards_scan_topk_after_masked" : "vg_shards_scan_topk_after";
        scan_after = (after_scan_fn)dlsym(G.handle, sym);
        if (!scan_after) missing = sym;
    }
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked scans need a newer libvectorgpu.so).", fname, missing); goto out; }

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
    if (!set_mask || !scan || (has_after && !scan_after)) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(int64_t));
    c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)k * sizeof(double));
    if (!c->rowids || !c->distance) { rc = SQLITE_NOMEM; goto out; }

    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: every distance through the slab path (k = 0), filtered, sorted and cut here */
        int64_t held = 0;
        if (filter_n > 1) qsort(filter_owned, (size_t)filter_n, sizeof(int64_t), masked_i64_cmp);
        rc = masked_ooc_topk_ex(vt, fname, t, quantized, scan_query, k, has_filter, filter_ids, filter_n, has_after ? &after_dist : NULL, after_rowid,
                                c->rowids, c->distance, &held);
        if (rc != SQLITE_OK) goto out;
        c->stream_n = held;
        goto out;
    }

    /* the mask is state of the staged copy, which other connections may hold too: set it and scan inside one hold of the lock */
    if (quantized) quant_lock(t); else full_lock(t);
    {
        int got = 0;
        int64_t allowed = 0;
        if ((has_filter && set_mask(corpus, filter_ids, filter_n, &allowed) != VG_OK) ||
            (has_after ? scan_after(corpus, t->opt.v_distance, scan_query, k, after_dist, after_rowid, c->rowids, c->distance, &got)
                       : scan(corpus, t->opt.v_distance, scan_query, k, c->rowids, c->distance, &got)) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto unlock;
        }
        c->stream_n = got;
    }
unlock:
    if (quantized) quant_unlock(t); else full_unlock(t);
out:
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(filter_owned);
    return rc;
}

static int full_masked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_full_scan_filtered", 0, 1, 0); }
static int quant_masked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_quantize_scan_filtered", 1, 1, 0); }

static sqlite3_module full_masked_module = {0, 0, masked_connect, within_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_masked_filter,
                                            within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_masked_module = {0, 0, masked_connect, within_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_masked_filter,
                                             within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

/* vext_batch.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * vector_full_scan_batch / vector_quantize_scan_batch (the only additions to the SQL surface)
 */
/* ---- batched queries (SURVEY 8f-4; the reference has no multi-query entry point: its equivalent is nq separate
 * vector_full_scan statements).  vector_full_scan_batch(tbl, col, queries, k) / vector_quantize_scan_batch(...):
 *   queries  BLOB of nq * dim elements (query vectors back to back), or TEXT JSON array of arrays
 *   output   (query, id, distance): k rows per query, ordered by query number (0-based) then distance ascending
 * Each query's rows are what the single-query function returns for it; f32 DOT/COSINE batches run as one
 * matrix-core pass over the corpus (vg_scan_topk_batch), everything else as nq GPU scans. */

static int batch_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(tbl hidden, vector hidden, k hidden, memidx hidden, id, distance, query);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int batch_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 10.0;
    info->estimatedRows = 1000;
    info->idxNum = 2;
    map_constraints(info);
    /* rows come out as (query asc, distance asc): claim the order only when that is what was asked for */
    if (info->nOrderBy == 2 && info->aOrderBy[0].iColumn == COL_QUERY && !info->aOrderBy[0].desc &&
        info->aOrderBy[1].iColumn == COL_DISTANCE && !info->aOrderBy[1].desc) info->orderByConsumed = 1;
    if (info->nOrderBy == 1 && info->aOrderBy[0].iColumn == COL_QUERY && !info->aOrderBy[0].desc) info->orderByConsumed = 1;
    return SQLITE_OK;
}

/* "[[..],[..]]" -> nq vectors back to back; returns sqlite3_malloc'd buffer */
static void *batch_from_json(sqlite3_vtab *vt, int type, const char *json, int dim, int *nq_out) {
    const int es = elem_size(type);
    const char *p = json;
    while (*p && isspace((unsigned char)*p)) p++;
    if (*p != '[') { vtab_error(vt, "Malformed JSON: expected '[' at the beginning of the array."); return NULL; }
    p++;
    int cap = 0, nq = 0;
    char *buf = NULL;
    while (1) {
        while (*p && (isspace((unsigned char)*p) || *p == ',')) p++;
        if (*p == ']' || !*p) break;
        if (*p != '[') { vtab_error(vt, "Malformed JSON: expected an array of arrays."); sqlite3_free(buf); return NULL; }
        int sz = 0;
        void *one = vector_from_json(NULL, vt, type, p, &sz, dim);
        if (!one) { sqlite3_free(buf); return NULL; }
        if (nq == cap) {
            cap = cap ? cap * 2 : 16;
            char *nb = (char *)sqlite3_realloc64(buf, (sqlite3_uint64)cap * dim * es);
            if (!nb) { sqlite3_free(one); sqlite3_free(buf); return NULL; }
            buf = nb;
        }
        memcpy(buf + (size_t)nq * dim * es, one, (size_t)dim * es);
        sqlite3_free(one);
        nq++;
        while (*p && *p != ']') p++;
        if (*p == ']') p++;
    }
    *nq_out = nq;
    return buf;
}

/* the `queries` argument of a batch function: a BLOB of nq * dim elements (used in place) or a JSON array of arrays (*owned:
 * sqlite3_malloc'd).  nq = 0 with SQLITE_OK: an empty JSON array */
static int batch_queries_arg(scan_vtab *vt, const char *fname, table_ctx *t, sqlite3_value *arg, const uint8_t **queries, void **owned, int *nq) {
    const int dim = t->opt.v_dim;
    const int64_t qrow = (int64_t)dim * elem_size(t->opt.v_type);
    *owned = NULL;
    *nq = 0;
    if (sqlite3_value_type(arg) == SQLITE_TEXT) {
        *owned = batch_from_json(&vt->base, t->opt.v_type, (const char *)sqlite3_value_text(arg), dim, nq);
        if (!*owned && *nq == 0 && vt->base.zErrMsg) return SQLITE_ERROR;
        *queries = (const uint8_t *)*owned;
        return SQLITE_OK;
    }
    *queries = (const uint8_t *)sqlite3_value_blob(arg);
    const int64_t bytes = sqlite3_value_bytes(arg);
    if (!*queries || bytes == 0 || bytes % qrow != 0)
        return vtab_error(&vt->base, "%s: the query batch has %lld bytes, expected a multiple of %lld (dimension %d).", fname, (long long)bytes, (long long)qrow, dim);
    *nq = (int)(bytes / qrow);
    return SQLITE_OK;
}

/* nq queries -> the quantized table's element type (*out: sqlite3_malloc'd nq x dim bytes, the caller frees it on every path) */
static int batch_quantize_queries(scan_vtab *vt, const char *fname, table_ctx *t, const uint8_t *queries, int nq, uint8_t **out) {
    const int dim = t->opt.v_dim;
    const int64_t qrow = (int64_t)dim * elem_size(t->opt.v_type);
    *out = (uint8_t *)sqlite3_malloc64((sqlite3_uint64)nq * dim);
    if (!*out) return SQLITE_NOMEM;
    for (int i = 0; i < nq; ++i)
        if (G.quantize_query(t->opt.v_type, queries + (int64_t)i * qrow, dim, t->scale, t->offset, t->opt.q_type, *out + (int64_t)i * dim) != VG_OK)
            return vtab_error(&vt->base, "%s: %s", fname, gpu_error());
    return SQLITE_OK;
}

/* nq x kk results + counts -> the cursor's (query, id, distance) rows, by query number */
static int batch_emit(scan_cursor *c, int nq, int kk, const int64_t *ids, const double *dist, const int *counts) {
    int64_t total = 0;
    for (int i = 0; i < nq; ++i) total += counts[i];
    sqlite3_free(c->rowids); sqlite3_free(c->distance); sqlite3_free(c->query_no);
    c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)(total ? total : 1) * sizeof(int64_t));
    c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)(total ? total : 1) * sizeof(double));
    c->query_no = (int *)sqlite3_malloc64((sqlite3_uint64)(total ? total : 1) * sizeof(int));
    if (!c->rowids || !c->distance || !c->query_no) return SQLITE_NOMEM;
    int w = 0;
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < counts[i]; ++j, ++w) {
            c->rowids[w] = ids[(int64_t)i * kk + j];
            c->distance[w] = dist[(int64_t)i * kk + j];
            c->query_no[w] = i;
        }
    c->row_count = w;
    return SQLITE_OK;
}

static int batch_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->row_index = 0;
    c->row_count = 0;
    if (argc != 4) return vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, 4, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if (i < 2 && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 2 && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
    table_ctx *t = context_lookup(vt->ctx, tbl, col);
    if (!t) return vtab_error(&vt->base, "%s: unable to retrieve context.", fname);
    const int dim = t->opt.v_dim, es = elem_size(t->opt.v_type);
    const int64_t qrow = (int64_t)dim * es;

    const uint8_t *queries = NULL;
    void *owned = NULL;
    uint8_t *qquant = NULL;
    int64_t *ids = NULL;
    double *dist = NULL;
    int *counts = NULL;
    char *err = NULL;
    int nq = 0, rc = SQLITE_OK;
    rc = batch_queries_arg(vt, fname, t, argv[2], &queries, &owned, &nq);
    if (rc != SQLITE_OK) return rc;
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0 || nq == 0) { rc = (k == 0) ? SQLITE_DONE : SQLITE_OK; goto out; }
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }

    vg_shards *corpus = NULL;
    const void *scan_queries = queries;
    if (quantized) {
        char name[SQL_BUF];
        sqlite3_snprintf(sizeof(name), name, "vector0_%q_%q", tbl, col);
        if (!exists_in_master(vt->db, "table", name)) {
            rc = vtab_error(&vt->base, "Quantization table not found for table '%s' and column '%s'. Ensure that vector_quantize() has been called before using vector_quantize_scan().", tbl, col);
            goto out;
        }
        if (!t->quant_preloaded || !t->quant) rc = stage_quant(vt->db, t, 0, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        rc = batch_quantize_queries(vt, fname, t, queries, nq, &qquant);
        if (rc != SQLITE_OK) goto out;
        scan_queries = qquant;
        corpus = t->quant;
    } else {
        rc = stage_full(vt->db, vt->ctx, t, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "staging failed"); goto out; }
        corpus = t->full;
    }
    {
        const int ooc = quantized ? t->quant_ooc : t->full_ooc;
        const int64_t n = ooc ? (int64_t)k : G.corpus_rows(corpus);
        const int kk = (int)((int64_t)k < n ? (int64_t)k : (n > 0 ? n : 1));     /* never more than N rows per query */
        ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * kk * sizeof(int64_t));
        dist = (double *)sqlite3_malloc64((sqlite3_uint64)nq * kk * sizeof(double));
        counts = (int *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int));
        if (!ids || !dist || !counts) { rc = SQLITE_NOMEM; goto out; }
        if (ooc) {
            /* a table that does not fit the device: Q independent scans, each reading the table again - what Q calls of the reference's
             * vector_full_scan do (vext_staging.inc: ooc_plan) */
            const int64_t qstep = quantized ? (int64_t)dim : qrow;
            for (int i = 0; i < nq; ++i) {
                rc = quantized ? ooc_scan_quant(vt->db, t, (const uint8_t *)scan_queries + i * qstep, kk, ids + (int64_t)i * kk, dist + (int64_t)i * kk, &counts[i], NULL, NULL, NULL, &err)
                               : ooc_scan_full(vt->db, t, (const uint8_t *)scan_queries + i * qstep, kk, ids + (int64_t)i * kk, dist + (int64_t)i * kk, &counts[i], NULL, NULL, NULL, &err);
                if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "scan failed"); goto out; }
            }
        } else {
            if (quantized) quant_lock(t); else full_lock(t);            /* (a copy shared with other connections: one scan at a time) */
            const int brc = G.scan_topk_batch(corpus, t->opt.v_distance, scan_queries, nq, kk, ids, dist, counts);
            if (brc != VG_OK) rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            if (quantized) quant_unlock(t); else full_unlock(t);
            if (brc != VG_OK) goto out;
        }
        rc = batch_emit(c, nq, kk, ids, dist, counts);
    }
out:
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(ids);
    sqlite3_free(dist);
    sqlite3_free(counts);
    return rc;
}

static int full_batch_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return batch_filter_common(c, argc, argv, "vector_full_scan_batch", 0); }
static int quant_batch_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return batch_filter_common(c, argc, argv, "vector_quantize_scan_batch", 1); }

/* vext_batch_masked.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * masked batch scans: vector_full_scan_batch_filtered / vector_quantize_scan_batch_filtered(table, column, queries, k, filter) ->
 * (query, id, distance): for every query of the batch the k nearest rows among those the filter names, ordered by query number
 * (0-based), then (distance, scan position).  `queries` is the batch functions' argument (vext_batch.inc: a BLOB of nq * dim elements or
 * a JSON array of arrays), `filter` the filtered functions' (vext_masked.inc: ONE read-only SELECT yielding rowids, or a BLOB of packed
 * int64 rowids) - their helpers parse both.  Each query's rows are what vector_full_scan_filtered returns for it.
 * The row mask is state of the staged copy, which several connections may share: the mask is set and the WHOLE batch is scanned
 * inside one hold of full_lock / quant_lock (the reason: vext_masked.inc).  The engine shares every row load between 4 (2) queries and
 * reads only the batches of rows the filter reaches (vg_shards_scan_topk_batch_masked).  An out-of-core table answers query by query
 * through the filtered function's slab route: correct, not fast (INTEGRATION.md).
 */
enum { BMCOL_QUERY = 0, BMCOL_ID = 1, BMCOL_DISTANCE = 2, BMCOL_TBL = 3, BMCOL_FILTER = 7 };

static int bmasked_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, k hidden, filter hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int bmasked_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 10.0;
    info->estimatedRows = 1000;
    info->idxNum = 3;
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ) continue;
        if (c->iColumn >= BMCOL_TBL && c->iColumn <= BMCOL_FILTER) {
            info->aConstraintUsage[i].argvIndex = c->iColumn - BMCOL_TBL + 1;
            info->aConstraintUsage[i].omit = 1;
        }
    }
    /* rows come out as (query asc, distance asc): claim the order only when that is what was asked for */
    if (info->nOrderBy == 2 && info->aOrderBy[0].iColumn == BMCOL_QUERY && !info->aOrderBy[0].desc &&
        info->aOrderBy[1].iColumn == BMCOL_DISTANCE && !info->aOrderBy[1].desc) info->orderByConsumed = 1;
    if (info->nOrderBy == 1 && info->aOrderBy[0].iColumn == BMCOL_QUERY && !info->aOrderBy[0].desc) info->orderByConsumed = 1;
    return SQLITE_OK;
}

/* the engine's entry points, resolved like masked_resolve does: an engine without them still loads, the functions then say so */
typedef int (*bmasked_scan_fn)(vg_shards *, int, const void *, int, int, int64_t *, double *, int *);
static const char *bmasked_resolve(masked_set_fn *set, bmasked_scan_fn *scan) {
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    *set = (masked_set_fn)dlsym(G.handle, "vg_shards_set_mask_rowids");
    if (!*set) return "vg_shards_set_mask_rowids";
    *scan = (bmasked_scan_fn)dlsym(G.handle, "vg_shards_scan_topk_batch_masked");
    if (!*scan) return "vg_shards_scan_topk_batch_masked";
    return NULL;
}

static int bmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->row_index = 0;
    c->row_count = 0;
    if (argc != 5) return vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, 5, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if (i < 2 && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 4 && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: filter cannot be NULL.", fname);
        if ((i == 2 || i == 4) && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
    const char *tbl = (const char *)sqlite3_value_text(argv[0]);
    const char *col = (const char *)sqlite3_value_text(argv[1]);
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
    int64_t *filter_ids = NULL;
    int64_t filter_n = 0;
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
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0 || nq == 0) goto out;                                                     /* no rows, no device (decided here) */
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if (k > 64) { rc = vtab_error(&vt->base, "%s: k must not exceed 64.", fname); goto out; }

    /* the allowed rowids: before anything is staged - a refused filter runs nothing */
    rc = masked_filter_arg(vt, fname, argv[4], &filter_ids, &filter_n);
    if (rc != SQLITE_OK) goto out;

    masked_set_fn set_mask = NULL;
    bmasked_scan_fn scan = NULL;
    const char *missing = bmasked_resolve(&set_mask, &scan);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked batch scans need a newer libvectorgpu.so).", fname, missing); goto out; }

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
    if (!set_mask || !scan) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * k * sizeof(int64_t));
    dist = (double *)sqlite3_malloc64((sqlite3_uint64)nq * k * sizeof(double));
    counts = (int *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int));
    if (!ids || !dist || !counts) { rc = SQLITE_NOMEM; goto out; }
    memset(counts, 0, (size_t)nq * sizeof(int));

    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: query by query through the filtered function's route (every distance through the slab
         * path, filtered, sorted and cut on the host) - each query reads the table again */
        if (filter_n > 1) qsort(filter_ids, (size_t)filter_n, sizeof(int64_t), masked_i64_cmp);
        for (int i = 0; i < nq; ++i) {
            int64_t held = 0;
            rc = masked_ooc_topk(vt, fname, t, quantized, (const uint8_t *)scan_queries + i * qstep, k, filter_ids, filter_n,
                                 ids + (int64_t)i * k, dist + (int64_t)i * k, &held);
            if (rc != SQLITE_OK) goto out;
            counts[i] = (int)held;
        }
    } else {
        /* the mask is state of the staged copy, which other connections may hold too: set it and scan the batch inside one hold of the lock */
        int64_t allowed = 0;
        if (quantized) quant_lock(t); else full_lock(t);
        if (set_mask(corpus, filter_ids, filter_n, &allowed) != VG_OK ||
            scan(corpus, t->opt.v_distance, scan_queries, nq, k, ids, dist, counts) != VG_OK)
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
    sqlite3_free(filter_ids);
    return rc;
}

static int full_bmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bmasked_filter_common(c, argc, argv, "vector_full_scan_batch_filtered", 0); }
static int quant_bmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bmasked_filter_common(c, argc, argv, "vector_quantize_scan_batch_filtered", 1); }

static int bmasked_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == BMCOL_QUERY) sqlite3_result_int(ctx, c->query_no[c->row_index]);
    else if (col == BMCOL_ID) sqlite3_result_int64(ctx, (sqlite3_int64)c->rowids[c->row_index]);
    else if (col == BMCOL_DISTANCE) sqlite3_result_double(ctx, c->distance[c->row_index]);
    return SQLITE_OK;
}

static sqlite3_module full_bmasked_module = {0, 0, bmasked_connect, bmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_bmasked_filter,
                                             tvf_next, tvf_eof, bmasked_column, tvf_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_bmasked_module = {0, 0, bmasked_connect, bmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_bmasked_filter,
                                              tvf_next, tvf_eof, bmasked_column, tvf_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

/* vext_within.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * range scans: vector_full_scan_within / vector_quantize_scan_within(table, column, vector, radius [, limit]) -> (id, distance),
 * every row whose distance is <= radius, ordered by (distance, scan position).  Additions next to the batch functions: the
 * reference's form of the question is "... FROM vector_full_scan_stream(...) WHERE distance <= ?", N rows stepped to keep a handful.
 * Staging, locks, tracked changes and freshness are vector_full_scan's (stage_full / stage_quant); the compare-and-compact runs in
 * the engine's scan kernel (vg_shards_scan_within).  An out-of-core table answers through the slab path with k = 0 and a filter +
 * sort here: correct, not fast (INTEGRATION.md).
 */
enum { WCOL_ID = 0, WCOL_DISTANCE = 1, WCOL_TBL = 2, WCOL_LIMIT = 6 };

static int within_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, radius hidden, lim hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int within_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 1.0;
    info->estimatedRows = 100;
    info->orderByConsumed = 1;                   /* output is distance-ascending, like the top-k functions */
    info->idxNum = 1;
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ) continue;
        if (c->iColumn >= WCOL_TBL && c->iColumn <= WCOL_LIMIT) {
            info->aConstraintUsage[i].argvIndex = c->iColumn - WCOL_TBL + 1;
            info->aConstraintUsage[i].omit = 1;
        }
    }
    return SQLITE_OK;
}

/* the engine's range-scan entry points, resolved like vg_host_alloc: an engine without them still loads, the functions then say so */
typedef int (*within_scan_fn)(vg_shards *, int, const void *, double, int64_t, int64_t *, int64_t *);
typedef int (*within_fetch_fn)(const vg_shards *, int64_t, int64_t, int64_t *, double *);
static const char *within_resolve(within_scan_fn *scan, within_fetch_fn *fetch) {
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    *scan = (within_scan_fn)dlsym(G.handle, "vg_shards_scan_within");
    if (!*scan) return "vg_shards_scan_within";
    *fetch = (within_fetch_fn)dlsym(G.handle, "vg_shards_scan_within_fetch");
    if (!*fetch) return "vg_shards_scan_within_fetch";
    return NULL;
}

typedef struct { float d; int64_t pos; } within_hit;
static int within_hit_cmp(const void *a, const void *b) {
    const within_hit *x = (const within_hit *)a, *y = (const within_hit *)b;
    if (x->d < y->d) return -1;
    if (x->d > y->d) return 1;
    return (x->pos > y->pos) - (x->pos < y->pos);
}

static int within_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->stream_pos = 0;
    c->stream_n = 0;
    if (argc != 4 && argc != 5) return vtab_error(&vt->base, "%s expects 4 or 5 arguments, but %d were provided.", fname, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if (i < 2 && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 2 && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: radius cannot be NULL.", fname);
        if (i == 3 && t != SQLITE_FLOAT && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type REAL or INTEGER (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 4 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
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
    float *all_dist = NULL;
    int64_t *all_ids = NULL;
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
    const double radius = sqlite3_value_double(argv[3]);
    const int64_t limit = (argc == 5) ? (int64_t)sqlite3_value_int64(argv[4]) : -1;      /* -1: none */
    if (argc == 5 && limit < 0) { rc = vtab_error(&vt->base, "%s: limit must not be negative.", fname); goto out; }
    if (argc == 5 && limit == 0) goto out;                                               /* no rows (decided here, like k = 0) */
    if (radius != radius) { rc = vtab_error(&vt->base, "%s: radius cannot be NaN.", fname); goto out; }

    within_scan_fn scan = NULL;
    within_fetch_fn fetch = NULL;
    const char *missing = within_resolve(&scan, &fetch);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (range scans need a newer libvectorgpu.so).", fname, missing); goto out; }

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
    if (!scan || !fetch) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: every distance through the slab path (k = 0), filtered and sorted here */
        int got = 0;
        int64_t n = 0;
        rc = quantized ? ooc_scan_quant(vt->db, t, scan_query, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err)
                       : ooc_scan_full(vt->db, t, scan_query, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err);
        if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "scan failed"); goto out; }
        int64_t m = 0;
        for (int64_t i = 0; i < n; ++i) if ((double)all_dist[i] <= radius && all_dist[i] < INFINITY) ++m;
        within_hit *hits = (within_hit *)sqlite3_malloc64((sqlite3_uint64)(m > 0 ? m : 1) * sizeof(within_hit));
        if (!hits) { rc = SQLITE_NOMEM; goto out; }
        m = 0;
        for (int64_t i = 0; i < n; ++i)
            if ((double)all_dist[i] <= radius && all_dist[i] < INFINITY) { hits[m].d = all_dist[i]; hits[m].pos = i; ++m; }
        qsort(hits, (size_t)m, sizeof(within_hit), within_hit_cmp);
        const int64_t held = (limit > 0 && limit < m) ? limit : m;
        c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)(held > 0 ? held : 1) * sizeof(int64_t));
        c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)(held > 0 ? held : 1) * sizeof(double));
        if (!c->rowids || !c->distance) { sqlite3_free(hits); rc = SQLITE_NOMEM; goto out; }
        for (int64_t i = 0; i < held; ++i) { c->rowids[i] = all_ids[hits[i].pos]; c->distance[i] = (double)hits[i].d; }
        sqlite3_free(hits);
        c->stream_n = held;
        goto out;
    }

    /* a copy shared with other connections is scanned by one of them at a time (vext_shared.inc); the result lives on the handle,
     * so it is copied into the cursor before the lock goes */
    if (quantized) quant_lock(t); else full_lock(t);
    {
        int64_t matches = 0, held = 0;
        if (scan(corpus, t->opt.v_distance, scan_query, radius, limit > 0 ? limit : 0, &matches, &held) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto unlock;
        }
        c->rowids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)(held > 0 ? held : 1) * sizeof(int64_t));
        c->distance = (double *)sqlite3_malloc64((sqlite3_uint64)(held > 0 ? held : 1) * sizeof(double));
        if (!c->rowids || !c->distance) { rc = SQLITE_NOMEM; goto unlock; }
        if (held > 0 && fetch(corpus, 0, held, c->rowids, c->distance) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto unlock;
        }
        c->stream_n = held;
    }
unlock:
    if (quantized) quant_unlock(t); else full_unlock(t);
out:
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(all_dist);
    sqlite3_free(all_ids);
    return rc;
}

static int full_within_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return within_filter_common(c, argc, argv, "vector_full_scan_within", 0); }
static int quant_within_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return within_filter_common(c, argc, argv, "vector_quantize_scan_within", 1); }

/* the cursor holds (rowids, distance) arrays of stream_n rows; 64-bit counters: a radius may match every row of a large table */
static int within_next(sqlite3_vtab_cursor *cur) { ((scan_cursor *)cur)->stream_pos++; return SQLITE_OK; }
static int within_eof(sqlite3_vtab_cursor *cur) { scan_cursor *c = (scan_cursor *)cur; return c->stream_pos >= c->stream_n; }
static int within_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == WCOL_ID) sqlite3_result_int64(ctx, (sqlite3_int64)c->rowids[c->stream_pos]);
    else if (col == WCOL_DISTANCE) sqlite3_result_double(ctx, c->distance[c->stream_pos]);
    return SQLITE_OK;
}
static int within_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    scan_cursor *c = (scan_cursor *)cur;
    *out = (sqlite3_int64)c->rowids[c->stream_pos];
    return SQLITE_OK;
}

static sqlite3_module full_within_module = {0, 0, within_connect, within_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_within_filter,
                                            within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_within_module = {0, 0, within_connect, within_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_within_filter,
                                             within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

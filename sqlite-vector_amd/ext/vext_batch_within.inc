/* vext_batch_within.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * batch range scans: vector_full_scan_batch_within / vector_quantize_scan_batch_within(table, column, queries, radius [, limit]) ->
 * (query, id, distance): for every query of the batch every row whose distance is <= that query's radius, ordered by query number
 * (0-based), then (distance, scan position).  `queries` is the batch functions' argument (vext_batch.inc: a BLOB of nq * dim elements or
 * a JSON array of arrays); `radius` a REAL / INTEGER shared by all queries, or a JSON array of exactly nq numbers; `limit` is per query.
 * Each query's rows are what vector_full_scan_within returns for it and its radius.  Staging, locks, tracked changes and freshness are
 * vector_full_scan_within's; the engine shares every row load between 4 (2) queries (vg_shards_scan_within_batch).  An out-of-core
 * table answers query by query through the within function's slab route: correct, not fast (INTEGRATION.md).
 */
enum { BWCOL_QUERY = 0, BWCOL_ID = 1, BWCOL_DISTANCE = 2, BWCOL_TBL = 3, BWCOL_LIMIT = 7 };

static int bwithin_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, radius hidden, lim hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

static int bwithin_best_index(sqlite3_vtab *v, sqlite3_index_info *info) {
    info->estimatedCost = 10.0;
    info->estimatedRows = 1000;
    info->idxNum = 4;
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ) continue;
        if (c->iColumn >= BWCOL_TBL && c->iColumn <= BWCOL_LIMIT) {
            info->aConstraintUsage[i].argvIndex = c->iColumn - BWCOL_TBL + 1;
            info->aConstraintUsage[i].omit = 1;
        }
    }
    /* rows come out as (query asc, distance asc): claim the order only when that is what was asked for */
    if (info->nOrderBy == 2 && info->aOrderBy[0].iColumn == BWCOL_QUERY && !info->aOrderBy[0].desc &&
        info->aOrderBy[1].iColumn == BWCOL_DISTANCE && !info->aOrderBy[1].desc) info->orderByConsumed = 1;
    if (info->nOrderBy == 1 && info->aOrderBy[0].iColumn == BWCOL_QUERY && !info->aOrderBy[0].desc) info->orderByConsumed = 1;
    return SQLITE_OK;
}

/* the engine's entry points, resolved like bmasked_resolve does: an engine without them still loads, the functions then say so */
typedef int (*bwithin_scan_fn)(vg_shards *, int, const void *, int, const double *, int64_t, int64_t *, int64_t *);
typedef int (*bwithin_fetch_fn)(const vg_shards *, int, int64_t, int64_t, int64_t *, double *);
static const char *bwithin_resolve(bwithin_scan_fn *scan, bwithin_fetch_fn *fetch) {
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    *scan = (bwithin_scan_fn)dlsym(G.handle, "vg_shards_scan_within_batch");
    if (!*scan) return "vg_shards_scan_within_batch";
    *fetch = (bwithin_fetch_fn)dlsym(G.handle, "vg_shards_scan_within_batch_fetch");
    if (!*fetch) return "vg_shards_scan_within_batch_fetch";
    return NULL;
}

/* one JSON number at p (-?digits[.digits][(e|E)[+-]digits]: no hex, no inf / nan, no leading '+'): its end, or NULL */
static const char *bwithin_json_number(const char *p) {
    if (*p == '-') p++;
    if (!isdigit((unsigned char)*p)) return NULL;
    while (isdigit((unsigned char)*p)) p++;
    if (*p == '.') {
        p++;
        if (!isdigit((unsigned char)*p)) return NULL;
        while (isdigit((unsigned char)*p)) p++;
    }
    if (*p == 'e' || *p == 'E') {
        p++;
        if (*p == '+' || *p == '-') p++;
        if (!isdigit((unsigned char)*p)) return NULL;
        while (isdigit((unsigned char)*p)) p++;
    }
    return p;
}

/* the `radius` argument: a number for every query, or a JSON array of exactly nq numbers (*out: sqlite3_malloc'd, nq doubles) */
static int bwithin_radius_arg(scan_vtab *vt, const char *fname, sqlite3_value *arg, int nq, double **out) {
    double *r = (double *)sqlite3_malloc64((sqlite3_uint64)(nq > 0 ? nq : 1) * sizeof(double));
    if (!r) return SQLITE_NOMEM;
    *out = r;
    if (sqlite3_value_type(arg) != SQLITE_TEXT) {
        const double v = sqlite3_value_double(arg);
        for (int i = 0; i < nq; ++i) r[i] = v;
    } else {
        const char *p = (const char *)sqlite3_value_text(arg);
        int n = 0, bad = 0;
        while (*p && isspace((unsigned char)*p)) p++;
        if (*p != '[') bad = 1;
        else p++;
        while (!bad && *p && isspace((unsigned char)*p)) p++;
        if (!bad && *p == ']') p++;                      /* an empty array */
        else while (!bad) {
            const char *end = bwithin_json_number(p);
            if (!end) { bad = 1; break; }
            const double v = strtod(p, NULL);            /* (the span is a plain decimal number: strtod reads exactly it) */
            if (n < nq) r[n] = v;
            ++n;
            p = end;
            while (*p && isspace((unsigned char)*p)) p++;
            if (*p == ']') { p++; break; }
            if (*p != ',') { bad = 1; break; }
            p++;                                         /* a comma: another number must follow */
            while (*p && isspace((unsigned char)*p)) p++;
        }
        while (!bad && *p && isspace((unsigned char)*p)) p++;
        if (bad || *p) return vtab_error(&vt->base, "%s: radius must be a number or a JSON array of numbers.", fname);
        if (n != nq) return vtab_error(&vt->base, "%s: the radius array has %d values, expected %d (one per query).", fname, n, nq);
    }
    for (int i = 0; i < nq; ++i)
        if (r[i] != r[i]) return vtab_error(&vt->base, "%s: radius cannot be NaN.", fname);
    return SQLITE_OK;
}

/* room for `more` further rows in the cursor's three arrays (they hold stream_n rows, *cap allocated) */
static int bwithin_reserve(scan_cursor *c, int64_t *cap, int64_t more) {
    const int64_t need = c->stream_n + more;
    if (need <= *cap && c->rowids) return SQLITE_OK;
    int64_t ncap = *cap ? *cap : 64;
    while (ncap < need) ncap *= 2;
    int64_t *ids = (int64_t *)sqlite3_realloc64(c->rowids, (sqlite3_uint64)ncap * sizeof(int64_t));
    if (ids) c->rowids = ids;
    double *dist = (double *)sqlite3_realloc64(c->distance, (sqlite3_uint64)ncap * sizeof(double));
    if (dist) c->distance = dist;
    int *qn = (int *)sqlite3_realloc64(c->query_no, (sqlite3_uint64)ncap * sizeof(int));
    if (qn) c->query_no = qn;
    if (!ids || !dist || !qn) return SQLITE_NOMEM;
    *cap = ncap;
    return SQLITE_OK;
}

static int bwithin_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
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
        if (i == 3 && t != SQLITE_FLOAT && t != SQLITE_INTEGER && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type REAL, INTEGER or TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 4 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
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
    uint8_t *qquant = NULL;
    double *radii = NULL;
    int64_t *matches = NULL, *held = NULL;
    float *all_dist = NULL;
    int64_t *all_ids = NULL;
    char *err = NULL;
    int nq = 0;
    int locked = 0;
    int64_t cap = 0;
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
    const int64_t limit = (argc == 5) ? (int64_t)sqlite3_value_int64(argv[4]) : -1;      /* -1: none */
    if (argc == 5 && limit < 0) { rc = vtab_error(&vt->base, "%s: limit must not be negative.", fname); goto out; }
    rc = bwithin_radius_arg(vt, fname, argv[3], nq, &radii);
    if (rc != SQLITE_OK) goto out;
    if ((argc == 5 && limit == 0) || nq == 0) goto out;                                  /* no rows, no device (decided here) */

    bwithin_scan_fn scan = NULL;
    bwithin_fetch_fn fetch = NULL;
    const char *missing = bwithin_resolve(&scan, &fetch);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (batch range scans need a newer libvectorgpu.so).", fname, missing); goto out; }

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
    if (!scan || !fetch) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    sqlite3_free(c->query_no); c->query_no = NULL;
    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: query by query, every distance through the slab path (k = 0), filtered and sorted here -
         * each query reads the table again */
        if ((rc = bwithin_reserve(c, &cap, 1)) != SQLITE_OK) goto out;
        for (int q = 0; q < nq; ++q) {
            int got = 0;
            int64_t n = 0;
            sqlite3_free(all_dist); all_dist = NULL;
            sqlite3_free(all_ids); all_ids = NULL;
            const uint8_t *one = (const uint8_t *)scan_queries + q * qstep;
            rc = quantized ? ooc_scan_quant(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err)
                           : ooc_scan_full(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err);
            if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "scan failed"); goto out; }
            int64_t m = 0;
            for (int64_t i = 0; i < n; ++i) if ((double)all_dist[i] <= radii[q] && all_dist[i] < INFINITY) ++m;
            within_hit *hits = (within_hit *)sqlite3_malloc64((sqlite3_uint64)(m > 0 ? m : 1) * sizeof(within_hit));
            if (!hits) { rc = SQLITE_NOMEM; goto out; }
            m = 0;
            for (int64_t i = 0; i < n; ++i)
                if ((double)all_dist[i] <= radii[q] && all_dist[i] < INFINITY) { hits[m].d = all_dist[i]; hits[m].pos = i; ++m; }
            qsort(hits, (size_t)m, sizeof(within_hit), within_hit_cmp);
            const int64_t keep = (limit > 0 && limit < m) ? limit : m;
            if ((rc = bwithin_reserve(c, &cap, keep)) != SQLITE_OK) { sqlite3_free(hits); goto out; }
            for (int64_t i = 0; i < keep; ++i) {
                c->rowids[c->stream_n] = all_ids[hits[i].pos];
                c->distance[c->stream_n] = (double)hits[i].d;
                c->query_no[c->stream_n] = q;
                ++c->stream_n;
            }
            sqlite3_free(hits);
        }
        goto out;
    }

    matches = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int64_t));
    held = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int64_t));
    if (!matches || !held) { rc = SQLITE_NOMEM; goto out; }
    /* a copy shared with other connections is scanned by one of them at a time (vext_shared.inc); the result lives on the handle,
     * so it is copied into the cursor before the lock goes */
    if (quantized) quant_lock(t); else full_lock(t);
    locked = 1;
    if (scan(corpus, t->opt.v_distance, scan_queries, nq, radii, limit > 0 ? limit : 0, matches, held) != VG_OK) {
        rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
        goto out;
    }
    {
        int64_t total = 0;
        for (int q = 0; q < nq; ++q) total += held[q];
        if ((rc = bwithin_reserve(c, &cap, total > 0 ? total : 1)) != SQLITE_OK) goto out;
        for (int q = 0; q < nq; ++q) {
            if (held[q] > 0 && fetch(corpus, q, 0, held[q], c->rowids + c->stream_n, c->distance + c->stream_n) != VG_OK) {
                rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
                c->stream_n = 0;
                goto out;
            }
            for (int64_t i = 0; i < held[q]; ++i) c->query_no[c->stream_n + i] = q;
            c->stream_n += held[q];
        }
    }
out:
    if (locked) { if (quantized) quant_unlock(t); else full_unlock(t); }
    if (rc != SQLITE_OK) c->stream_n = 0;
    sqlite3_free(err);
    sqlite3_free(owned);
    sqlite3_free(qquant);
    sqlite3_free(radii);
    sqlite3_free(matches);
    sqlite3_free(held);
    sqlite3_free(all_dist);
    sqlite3_free(all_ids);
    return rc;
}

static int full_bwithin_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bwithin_filter_common(c, argc, argv, "vector_full_scan_batch_within", 0); }
static int quant_bwithin_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return bwithin_filter_common(c, argc, argv, "vector_quantize_scan_batch_within", 1); }

/* the cursor holds (query_no, rowids, distance) arrays of stream_n rows (64-bit counters, as in vext_within.inc) */
static int bwithin_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == BWCOL_QUERY) sqlite3_result_int(ctx, c->query_no[c->stream_pos]);
    else if (col == BWCOL_ID) sqlite3_result_int64(ctx, (sqlite3_int64)c->rowids[c->stream_pos]);
    else if (col == BWCOL_DISTANCE) sqlite3_result_double(ctx, c->distance[c->stream_pos]);
    return SQLITE_OK;
}
static int bwithin_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = (sqlite3_int64)((scan_cursor *)cur)->stream_pos;
    return SQLITE_OK;
}

static sqlite3_module full_bwithin_module = {0, 0, bwithin_connect, bwithin_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_bwithin_filter,
                                             within_next, within_eof, bwithin_column, bwithin_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_bwithin_module = {0, 0, bwithin_connect, bwithin_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_bwithin_filter,
                                              within_next, within_eof, bwithin_column, bwithin_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

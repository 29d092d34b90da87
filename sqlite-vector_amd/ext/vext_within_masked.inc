/* vext_within_masked.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * masked range scans: vector_full_scan_within_filtered / vector_quantize_scan_within_filtered(table, column, vector, radius, filter
 * [, limit]) -> (id, distance), every row AMONG THOSE THE FILTER NAMES whose distance is <= radius, ordered by (distance, scan
 * position).  `filter` is the masked functions' argument (vext_masked.inc: ONE read-only SELECT whose first column yields rowids, or a
 * BLOB of packed little-endian int64 rowids; NULL is refused); radius and limit are the within functions' (vext_within.inc).  The
 * question it answers is "... FROM vector_full_scan_stream(...) WHERE id IN (<filter>) AND distance <= r ORDER BY distance [LIMIT n]"
 * without writing, copying and stepping N rows.
 * Staging, locks, tracked changes and freshness are vector_full_scan's (stage_full / stage_quant).  The row mask is state of the staged
 * copy, and a copy may be shared by several connections: the mask is set and the scan runs inside ONE hold of full_lock / quant_lock,
 * as in vext_masked.inc.  An out-of-core table answers through the slab path with k = 0 and a filter + sort here: correct, not fast
 * (INTEGRATION.md).  Cursor and columns are the within functions'.  What follows the argument parsing - resolve, stage, out-of-core or
 * lock + mask + scan + fetch - is ONE routine (wmasked_run) that serves the batch form (vext_batch_within_masked.inc) too: the single
 * form is a batch of one that calls the engine's single entry points.
 */
enum { WMCOL_LIMIT = 7, BWMCOL_LIMIT = 8 };

static int wmasked_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    int rc = sqlite3_declare_vtab(db, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, radius hidden, filter hidden, lim hidden);");
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}

/* `base`'s index plan plus one more hidden argument column (`last`, the argument behind base's last one) */
static int wmasked_plan(sqlite3_vtab *v, sqlite3_index_info *info, int (*base)(sqlite3_vtab *, sqlite3_index_info *), int first, int last) {
    int rc = base(v, info);
    for (int i = 0; rc == SQLITE_OK && i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ || c->iColumn != last) continue;
        info->aConstraintUsage[i].argvIndex = last - first + 1;
        info->aConstraintUsage[i].omit = 1;
    }
    return rc;
}
static int wmasked_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return wmasked_plan(v, info, within_best_index, WCOL_TBL, WMCOL_LIMIT); }

/* the engine's entry points of both forms, resolved like the range scans': an engine without them still loads, the functions then say so */
typedef struct {
    masked_set_fn set_mask;
    within_scan_fn scan;              /* single form */
    within_fetch_fn fetch;
    bwithin_scan_fn bscan;            /* batch form */
    bwithin_fetch_fn bfetch;
} wmasked_fns;
static const char *wmasked_resolve(int batch, wmasked_fns *f) {
    memset(f, 0, sizeof(*f));
    if (!gpu_load()) return NULL;                /* (no engine at all: the staging step reports why) */
    f->set_mask = (masked_set_fn)dlsym(G.handle, "vg_shards_set_mask_rowids");
    if (!f->set_mask) return "vg_shards_set_mask_rowids";
    if (batch) {
        f->bscan = (bwithin_scan_fn)dlsym(G.handle, "vg_shards_scan_within_batch_masked");
        if (!f->bscan) return "vg_shards_scan_within_batch_masked";
        f->bfetch = (bwithin_fetch_fn)dlsym(G.handle, "vg_shards_scan_within_batch_fetch");
        if (!f->bfetch) return "vg_shards_scan_within_batch_fetch";
    } else {
        f->scan = (within_scan_fn)dlsym(G.handle, "vg_shards_scan_within_masked");
        if (!f->scan) return "vg_shards_scan_within_masked";
        f->fetch = (within_fetch_fn)dlsym(G.handle, "vg_shards_scan_within_fetch");
        if (!f->fetch) return "vg_shards_scan_within_fetch";
    }
    return NULL;
}

/* one query against a table that does not fit the device: every distance through the slab path (k = 0), filtered against the SORTED
 * rowids and the radius, sorted by (distance, scan position), cut to `limit` and appended to the cursor's rows as query `q` */
static int wmasked_ooc_query(scan_vtab *vt, const char *fname, table_ctx *t, int quantized, const void *one, double radius, int64_t limit,
                             const int64_t *sorted_ids, int64_t filter_n, scan_cursor *c, int64_t *cap, int q) {
    char *err = NULL;
    float *all_dist = NULL;
    int64_t *all_ids = NULL;
    within_hit *hits = NULL;
    int got = 0;
    int64_t n = 0, m = 0;
    int rc = quantized ? ooc_scan_quant(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err)
                       : ooc_scan_full(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &err);
    if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, err ? err : "scan failed"); goto done; }
    hits = (within_hit *)sqlite3_malloc64((sqlite3_uint64)(n > 0 ? n : 1) * sizeof(within_hit));
    if (!hits) { rc = SQLITE_NOMEM; goto done; }
    for (int64_t i = 0; i < n && filter_n > 0; ++i) {
        if (!((double)all_dist[i] <= radius && all_dist[i] < INFINITY)) continue;        /* NaN / +Inf never match */
        if (!bsearch(&all_ids[i], sorted_ids, (size_t)filter_n, sizeof(int64_t), masked_i64_cmp)) continue;
        hits[m].d = all_dist[i]; hits[m].pos = i; ++m;
    }
    qsort(hits, (size_t)m, sizeof(within_hit), within_hit_cmp);
    const int64_t keep = (limit > 0 && limit < m) ? limit : m;
    if ((rc = bwithin_reserve(c, cap, keep > 0 ? keep : 1)) != SQLITE_OK) goto done;
    for (int64_t i = 0; i < keep; ++i) {
        c->rowids[c->stream_n] = all_ids[hits[i].pos];
        c->distance[c->stream_n] = (double)hits[i].d;
        c->query_no[c->stream_n] = q;
        ++c->stream_n;
    }
done:
    sqlite3_free(hits);
    sqlite3_free(err);
    sqlite3_free(all_dist);
    sqlite3_free(all_ids);
    return rc;
}

/* nq queries (element type of the table, row-major), a radius each, limit (-1: none; never 0), the filter argument -> the cursor's
 * (query_no, rowids, distance) rows.  batch = 0: nq is 1 and the engine's single entry points answer. */
static int wmasked_run(scan_cursor *c, scan_vtab *vt, const char *fname, table_ctx *t, int quantized, int batch, const uint8_t *queries, int nq,
                       const double *radii, int64_t limit, sqlite3_value *filter) {
    int rc = SQLITE_OK;
    char *err = NULL;
    uint8_t *qquant = NULL;
    int64_t *filter_ids = NULL, *matches = NULL, *held = NULL;
    int64_t filter_n = 0, cap = 0;
    int locked = 0;
    const int dim = t->opt.v_dim;
    int64_t qstep = (int64_t)dim * elem_size(t->opt.v_type);

    /* the allowed rowids: before anything is staged - a refused filter runs nothing */
    rc = masked_filter_arg(vt, fname, filter, &filter_ids, &filter_n);
    if (rc != SQLITE_OK) goto out;

    wmasked_fns f;
    const char *missing = wmasked_resolve(batch, &f);
    if (missing) { rc = vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked range scans need a newer libvectorgpu.so).", fname, missing); goto out; }

    vg_shards *corpus = NULL;
    const uint8_t *scan_queries = queries;
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
    if (!f.set_mask) { rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error()); goto out; }

    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    sqlite3_free(c->query_no); c->query_no = NULL;
    if (quantized ? t->quant_ooc : t->full_ooc) {
        /* the table does not fit the device: query by query - each reads the table again */
        if (filter_n > 1) qsort(filter_ids, (size_t)filter_n, sizeof(int64_t), masked_i64_cmp);
        for (int q = 0; q < nq && rc == SQLITE_OK; ++q)
            rc = wmasked_ooc_query(vt, fname, t, quantized, scan_queries + q * qstep, radii[q], limit, filter_ids, filter_n, c, &cap, q);
        goto out;
    }

    matches = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int64_t));
    held = (int64_t *)sqlite3_malloc64((sqlite3_uint64)nq * sizeof(int64_t));
    if (!matches || !held) { rc = SQLITE_NOMEM; goto out; }
    /* the mask is state of the staged copy, which other connections may hold too: set it, scan, and copy the result (it lives on the
     * handle) into the cursor inside one hold of the lock */
    if (quantized) quant_lock(t); else full_lock(t);
    locked = 1;
    {
        int64_t allowed = 0, total = 0;
        const int64_t lim = limit > 0 ? limit : 0;
        if (f.set_mask(corpus, filter_ids, filter_n, &allowed) != VG_OK ||
            (batch ? f.bscan(corpus, t->opt.v_distance, scan_queries, nq, radii, lim, matches, held)
                   : f.scan(corpus, t->opt.v_distance, scan_queries, radii[0], lim, matches, held)) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        for (int q = 0; q < nq; ++q) total += held[q];
        if ((rc = bwithin_reserve(c, &cap, total > 0 ? total : 1)) != SQLITE_OK) goto out;
        for (int q = 0; q < nq; ++q) {
            if (held[q] > 0 && (batch ? f.bfetch(corpus, q, 0, held[q], c->rowids + c->stream_n, c->distance + c->stream_n)
                                      : f.fetch(corpus, 0, held[q], c->rowids + c->stream_n, c->distance + c->stream_n)) != VG_OK) {
                rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
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
    sqlite3_free(qquant);
    sqlite3_free(filter_ids);
    sqlite3_free(matches);
    sqlite3_free(held);
    return rc;
}

/* the types of the arguments both forms share: (table, column, vector | queries, radius, filter [, limit]); radius may be TEXT (a JSON
 * array) in the batch form only */
static int wmasked_arg_types(scan_vtab *vt, const char *fname, int argc, sqlite3_value **argv, int batch) {
    if (argc != 5 && argc != 6) return vtab_error(&vt->base, "%s expects 5 or 6 arguments, but %d were provided.", fname, argc);
    for (int i = 0; i < argc; ++i) {
        int t = sqlite3_value_type(argv[i]);
        if (i < 2 && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 4 && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: filter cannot be NULL.", fname);
        if ((i == 2 || i == 4) && t != SQLITE_TEXT && t != SQLITE_BLOB) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: radius cannot be NULL.", fname);
        if (i == 3 && !batch && t != SQLITE_FLOAT && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type REAL or INTEGER (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 3 && batch && t != SQLITE_FLOAT && t != SQLITE_INTEGER && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type REAL, INTEGER or TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (i == 5 && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
    }
    return SQLITE_OK;
}

static int wmasked_quant_table_check(scan_vtab *vt, const char *fname, const char *tbl, const char *col) {
    char name[SQL_BUF];
    sqlite3_snprintf(sizeof(name), name, "vector0_%q_%q", tbl, col);
    if (exists_in_master(vt->db, "table", name)) return SQLITE_OK;
    return vtab_error(&vt->base, "Quantization table not found for table '%s' and column '%s'. Ensure that vector_quantize() has been called before using %s().", tbl, col, fname);
}

static int wmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    scan_cursor *c = (scan_cursor *)cur;
    scan_vtab *vt = (scan_vtab *)cur->pVtab;
    c->streaming = 0;
    c->stream_pos = 0;
    c->stream_n = 0;
    int rc = wmasked_arg_types(vt, fname, argc, argv, 0);
    if (rc != SQLITE_OK) return rc;
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
    if (qbytes < t->opt.v_dim * elem_size(t->opt.v_type)) {
        rc = vtab_error(&vt->base, "%s: query vector has %d bytes, expected %d.", fname, qbytes, t->opt.v_dim * elem_size(t->opt.v_type));
        goto out;
    }
    if (quantized && (rc = wmasked_quant_table_check(vt, fname, tbl, col)) != SQLITE_OK) goto out;
    const double radius = sqlite3_value_double(argv[3]);
    const int64_t limit = (argc == 6) ? (int64_t)sqlite3_value_int64(argv[5]) : -1;      /* -1: none */
    if (argc == 6 && limit < 0) { rc = vtab_error(&vt->base, "%s: limit must not be negative.", fname); goto out; }
    if (radius != radius) { rc = vtab_error(&vt->base, "%s: radius cannot be NaN.", fname); goto out; }
    if (argc == 6 && limit == 0) goto out;                                               /* no rows (decided here, like k = 0) */
    rc = wmasked_run(c, vt, fname, t, quantized, 0, (const uint8_t *)query, 1, &radius, limit, argv[4]);
out:
    sqlite3_free(owned);
    return rc;
}

static int full_wmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return wmasked_filter_common(c, argc, argv, "vector_full_scan_within_filtered", 0); }
static int quant_wmasked_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return wmasked_filter_common(c, argc, argv, "vector_quantize_scan_within_filtered", 1); }

static sqlite3_module full_wmasked_module = {0, 0, wmasked_connect, wmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_wmasked_filter,
                                             within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_wmasked_module = {0, 0, wmasked_connect, wmasked_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_wmasked_filter,
                                              within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

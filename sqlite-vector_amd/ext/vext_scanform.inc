/* vext_scanform.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * what every table-valued scan function shares, once: connect, the index plan, the argument-type table, the steps of one call
 * (open / stage / lock / close), the engine-symbol resolver, the out-of-core answer of one query, the rows of a range scan into the
 * cursor, the module table.  Nothing here knows a form: schema texts, argument specs, value checks and engine calls are the form
 * files' (vext_tvf, vext_batch, vext_range, vext_topk, vext_labeled).
 */

/* ------------------------------------------------------------------------------------------------ connect, modules */

static int scan_vtab_connect(sqlite3 *db, void *aux, sqlite3_vtab **out, const char *decl) {
    int rc = sqlite3_declare_vtab(db, decl);
    if (rc != SQLITE_OK) return rc;
    scan_vtab *v = (scan_vtab *)sqlite3_malloc(sizeof(scan_vtab));
    if (!v) return SQLITE_NOMEM;
    memset(v, 0, sizeof(*v));
    v->db = db;
    v->ctx = (vec_context *)aux;
    *out = &v->base;
    return SQLITE_OK;
}
#define SCAN_CONNECT(name, decl) \
    static int name(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) { return scan_vtab_connect(db, aux, out, decl); }

/* a form's two modules, vector_full_scan<suffix> and vector_quantize_scan<suffix>: common(cursor, argc, argv, name, quantized) is its xFilter */
#define SCAN_MODULE(name, connect, best_index, filter, next, eof, column, rowid) \
    static sqlite3_module name = {0, 0, connect, best_index, tvf_disconnect, 0, tvf_open, tvf_close, filter, next, eof, column, rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SCAN_FORM(stem, suffix, common, connect, best_index, next, eof, column, rowid) \
    static int full_##stem##_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return common(c, argc, argv, "vector_full_scan" suffix, 0); } \
    static int quant_##stem##_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return common(c, argc, argv, "vector_quantize_scan" suffix, 1); } \
    SCAN_MODULE(full_##stem##_module, connect, best_index, full_##stem##_filter, next, eof, column, rowid); \
    SCAN_MODULE(quant_##stem##_module, connect, best_index, quant_##stem##_filter, next, eof, column, rowid)

/* ------------------------------------------------------------------------------------------------ index plans */

/* the hidden argument columns [first..last] go to xFilter in order */
static void plan_args(sqlite3_index_info *info, int first, int last) {
    for (int i = 0; i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ || c->iColumn < first || c->iColumn > last) continue;
        info->aConstraintUsage[i].argvIndex = c->iColumn - first + 1;
        info->aConstraintUsage[i].omit = 1;
    }
}

static int plan_single(sqlite3_index_info *info, int idx_num, int first, int last) {
    info->estimatedCost = 1.0;
    info->estimatedRows = 100;
    info->orderByConsumed = 1;                   /* output is distance-ascending (sqlite-vector.c:1853) */
    info->idxNum = idx_num;
    plan_args(info, first, last);
    return SQLITE_OK;
}

static int plan_batch(sqlite3_index_info *info, int idx_num, int first, int last, int col_query, int col_distance) {
    info->estimatedCost = 10.0;
    info->estimatedRows = 1000;
    info->idxNum = idx_num;
    plan_args(info, first, last);
    /* rows come out as (query asc, distance asc): claim the order only when that is what was asked for */
    if (info->nOrderBy == 2 && info->aOrderBy[0].iColumn == col_query && !info->aOrderBy[0].desc &&
        info->aOrderBy[1].iColumn == col_distance && !info->aOrderBy[1].desc) info->orderByConsumed = 1;
    if (info->nOrderBy == 1 && info->aOrderBy[0].iColumn == col_query && !info->aOrderBy[0].desc) info->orderByConsumed = 1;
    return SQLITE_OK;
}

/* the added forms' layouts (vext_cursor.inc): a module has no column behind its own last one, so the longest form's bound serves all */
static int single_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return plan_single(info, 1, WCOL_TBL, WCOL_LAST); }
static int btopk_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return plan_batch(info, 3, BCOL_TBL, BCOL_LAST, BCOL_QUERY, BCOL_DISTANCE); }
static int brange_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return plan_batch(info, 4, BCOL_TBL, BCOL_LAST, BCOL_QUERY, BCOL_DISTANCE); }

/* ------------------------------------------------------------------------------------------------ argument types */

/* what one argument may be.  ARG_ANY: the form checks it itself, behind the table (such arguments are the last ones) */
enum { ARG_ANY = 0, ARG_TEXT, ARG_VECTOR, ARG_INTEGER, ARG_NUMBER, ARG_NUMBER_OR_JSON, ARG_FILTER };
typedef struct {
    int n;                             /* arguments */
    const char *or_one_more;           /* NULL, or: n + 1 are fine too (the last one optional) - the message for any other count */
    unsigned char kind[8];
} arg_spec;

/* count, then the arguments in order: the first bad one is reported; at one position NULL is refused by name before the type is */
static int scan_check_args(scan_vtab *vt, const char *fname, const arg_spec *spec, int argc, sqlite3_value **argv) {
    if (spec->or_one_more ? (argc != spec->n && argc != spec->n + 1) : argc != spec->n)
        return spec->or_one_more ? vtab_error(&vt->base, spec->or_one_more, fname, argc)
                                 : vtab_error(&vt->base, "%s expects %d arguments, but %d were provided.", fname, spec->n, argc);
    for (int i = 0; i < argc; ++i) {
        const int t = sqlite3_value_type(argv[i]), kind = spec->kind[i];
        if (kind == ARG_TEXT && t != SQLITE_TEXT) return vtab_error(&vt->base, "%s: argument %d must be of type TEXT (got %s).", fname, i + 1, sql_type_name(t));
        if (kind == ARG_FILTER && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: filter cannot be NULL.", fname);
        if ((kind == ARG_VECTOR || kind == ARG_FILTER) && t != SQLITE_TEXT && t != SQLITE_BLOB)
            return vtab_error(&vt->base, "%s: argument %d must be of type TEXT or BLOB (got %s).", fname, i + 1, sql_type_name(t));
        if (kind == ARG_INTEGER && t != SQLITE_INTEGER) return vtab_error(&vt->base, "%s: argument %d must be of type INTEGER (got %s).", fname, i + 1, sql_type_name(t));
        if ((kind == ARG_NUMBER || kind == ARG_NUMBER_OR_JSON) && t == SQLITE_NULL) return vtab_error(&vt->base, "%s: radius cannot be NULL.", fname);
        if (kind == ARG_NUMBER && t != SQLITE_FLOAT && t != SQLITE_INTEGER)
            return vtab_error(&vt->base, "%s: argument %d must be of type REAL or INTEGER (got %s).", fname, i + 1, sql_type_name(t));
        if (kind == ARG_NUMBER_OR_JSON && t != SQLITE_FLOAT && t != SQLITE_INTEGER && t != SQLITE_TEXT)
            return vtab_error(&vt->base, "%s: argument %d must be of type REAL, INTEGER or TEXT (got %s).", fname, i + 1, sql_type_name(t));
    }
    return SQLITE_OK;
}

/* ------------------------------------------------------------------------------------------------ the batch argument, the batch rows */

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

/* nq x kk results + counts -> the cursor's (query, id, distance) rows, by query number (row_count and stream_n both say how many) */
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
    c->stream_n = w;
    return SQLITE_OK;
}

/* ------------------------------------------------------------------------------------------------ one call */

/* One xFilter call.  scan_begin, [scan_lookup,] scan_open, the form's own checks, [scan_resolve,] scan_stage, then either the
 * out-of-core answer (s.ooc) or scan_lock + the engine call; scan_close on every path behind scan_begin. */
typedef struct {
    scan_cursor *c;
    scan_vtab *vt;
    const char *fname, *tbl, *col;
    int quantized;
    table_ctx *t;
    const uint8_t *queries;            /* nq query vectors in the table's element type, back to back */
    int nq;
    vg_shards *corpus;                 /* behind scan_stage: the staged copy, the queries in ITS element type, their stride */
    const uint8_t *scan_queries;
    int64_t qstep;
    int ooc;                           /* the table does not fit the device: every scan reads it again, slab by slab (vext_staging.inc: ooc_plan) */
    int no_engine, locked;
    int64_t cap;                       /* rows allocated in the cursor (scan_rows_reserve) */
    void *owned;                       /* freed by scan_close */
    uint8_t *qquant;
    char *err;
    int64_t *ids;                      /* scan_topk_buffers: nq x k results and nq counts */
    double *dist;
    int *counts;
} scan_call;

static void scan_begin(scan_call *s, sqlite3_vtab_cursor *cur, const char *fname, int quantized, int streaming) {
    memset(s, 0, sizeof(*s));
    s->c = (scan_cursor *)cur;
    s->vt = (scan_vtab *)cur->pVtab;
    s->fname = fname;
    s->quantized = quantized;
    s->c->streaming = streaming;
    s->c->row_index = 0;
    s->c->row_count = 0;
    s->c->stream_pos = 0;
    s->c->stream_n = 0;
}

/* argv[0], argv[1] -> the table's context */
static int scan_lookup(scan_call *s, sqlite3_value **argv) {
    s->tbl = (const char *)sqlite3_value_text(argv[0]);
    s->col = (const char *)sqlite3_value_text(argv[1]);
    s->t = context_lookup(s->vt->ctx, s->tbl, s->col);
    if (!s->t) return vtab_error(&s->vt->base, "%s: unable to retrieve context.", s->fname);
    return SQLITE_OK;
}

/* the quantized functions need the table vector_quantize() writes; `called` is the function the message names */
static int scan_quant_table(scan_call *s, const char *called) {
    char name[SQL_BUF];
    if (!s->quantized) return SQLITE_OK;
    sqlite3_snprintf(sizeof(name), name, "vector0_%q_%q", s->tbl, s->col);
    if (exists_in_master(s->vt->db, "table", name)) return SQLITE_OK;
    return vtab_error(&s->vt->base, "Quantization table not found for table '%s' and column '%s'. Ensure that vector_quantize() has been called before using %s().", s->tbl, s->col, called);
}

/* the context (unless scan_lookup has it already), the query argument argv[2] - one vector, or a batch - with its length check, and
 * the quantization table (called = NULL: the form calls scan_quant_table itself, later) */
static int scan_open(scan_call *s, sqlite3_value **argv, int batch, const char *called) {
    scan_vtab *vt = s->vt;
    int rc = s->t ? SQLITE_OK : scan_lookup(s, argv);
    if (rc != SQLITE_OK) return rc;
    table_ctx *t = s->t;
    if (batch) {
        rc = batch_queries_arg(vt, s->fname, t, argv[2], &s->queries, &s->owned, &s->nq);
        if (rc != SQLITE_OK) return rc;
    } else {
        int qbytes = 0;
        if (sqlite3_value_type(argv[2]) == SQLITE_TEXT) {
            s->owned = vector_from_json(NULL, &vt->base, t->opt.v_type, (const char *)sqlite3_value_text(argv[2]), &qbytes, t->opt.v_dim);
            if (!s->owned) return SQLITE_ERROR;
            s->queries = (const uint8_t *)s->owned;
        } else {
            s->queries = (const uint8_t *)sqlite3_value_blob(argv[2]);
            qbytes = sqlite3_value_bytes(argv[2]);
            if (!s->queries) return vtab_error(&vt->base, "%s: input vector cannot be NULL.", s->fname);
        }
        /* the reference reads past a short query BLOB (:1774); refuse instead of faulting on the device */
        if (qbytes < t->opt.v_dim * elem_size(t->opt.v_type))
            return vtab_error(&vt->base, "%s: query vector has %d bytes, expected %d.", s->fname, qbytes, t->opt.v_dim * elem_size(t->opt.v_type));
        s->nq = 1;
    }
    return called ? scan_quant_table(s, called) : SQLITE_OK;
}

/* names[0..n) -> fns[0..n) in the engine; the first missing name in list order, or NULL.  No engine at all: NULL too - the staging
 * step reports why (and scan_stage fails in any case) */
static const char *scan_resolve(scan_call *s, const char *const *names, void **fns, int n) {
    memset(fns, 0, (size_t)n * sizeof(void *));
    if (!gpu_load()) { s->no_engine = 1; return NULL; }
    for (int i = 0; i < n; ++i)
        if (!(fns[i] = dlsym(G.handle, names[i]))) return names[i];
    return NULL;
}

/* the copy to scan (staged on first use, refreshed when the table moved) and the queries in its element type */
static int scan_stage(scan_call *s) {
    scan_vtab *vt = s->vt;
    table_ctx *t = s->t;
    const int dim = t->opt.v_dim;
    int rc = SQLITE_OK;
    s->scan_queries = s->queries;
    s->qstep = (int64_t)dim * elem_size(t->opt.v_type);
    if (s->quantized) {
        if (!t->quant_preloaded || !t->quant) rc = stage_quant(vt->db, t, 0, &s->err);   /* not preloaded: stage on first use */
        if (rc != SQLITE_OK) return vtab_error(&vt->base, "%s: %s", s->fname, s->err ? s->err : "staging failed");
        s->qquant = (uint8_t *)sqlite3_malloc64((sqlite3_uint64)s->nq * dim);
        if (!s->qquant) return SQLITE_NOMEM;
        /* the queries are quantized with the stored scale/offset on every scan (sqlite-vector.c:2166-2177) */
        for (int i = 0; i < s->nq; ++i)
            if (G.quantize_query(t->opt.v_type, s->queries + i * s->qstep, dim, t->scale, t->offset, t->opt.q_type, s->qquant + (int64_t)i * dim) != VG_OK)
                return vtab_error(&vt->base, "%s: %s", s->fname, gpu_error());
        s->scan_queries = s->qquant;
        s->qstep = dim;
        s->corpus = t->quant;
        s->ooc = t->quant_ooc;
    } else {
        rc = stage_full(vt->db, vt->ctx, t, &s->err);
        if (rc != SQLITE_OK) return vtab_error(&vt->base, "%s: %s", s->fname, s->err ? s->err : "staging failed");
        s->corpus = t->full;
        s->ooc = t->full_ooc;
    }
    if (s->no_engine) return vtab_error(&vt->base, "%s: %s", s->fname, gpu_error());
    return SQLITE_OK;
}

/* a copy shared with other connections is scanned by one of them at a time (vext_shared.inc).  Masks, labels and a range scan's
 * result are state of the copy: they are set, and the result is copied into the cursor, inside ONE hold */
static void scan_lock(scan_call *s) {
    table_ctx *t = s->t;
    const int quantized = s->quantized;
    if (quantized) quant_lock(t); else full_lock(t);
    s->locked = 1;
}
static void scan_unlock(scan_call *s) {
    if (!s->locked) return;
    if (s->quantized) quant_unlock(s->t); else full_unlock(s->t);
    s->locked = 0;
}

/* room for nq x kk results and nq counts */
static int scan_topk_buffers(scan_call *s, int kk) {
    s->ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)s->nq * kk * sizeof(int64_t));
    s->dist = (double *)sqlite3_malloc64((sqlite3_uint64)s->nq * kk * sizeof(double));
    s->counts = (int *)sqlite3_malloc64((sqlite3_uint64)s->nq * sizeof(int));
    if (!s->ids || !s->dist || !s->counts) return SQLITE_NOMEM;
    memset(s->counts, 0, (size_t)s->nq * sizeof(int));
    return SQLITE_OK;
}

/* gives the lock back and frees what the call owns; a failed call leaves no rows in the cursor.  Returns rc */
static int scan_close(scan_call *s, int rc) {
    scan_unlock(s);
    if (rc != SQLITE_OK) { s->c->stream_n = 0; s->c->row_count = 0; }
    sqlite3_free(s->err);
    sqlite3_free(s->owned);
    sqlite3_free(s->qquant);
    sqlite3_free(s->ids);
    sqlite3_free(s->dist);
    sqlite3_free(s->counts);
    return rc;
}

/* ------------------------------------------------------------------------------------------------ the out-of-core answer */

static int i64_cmp(const void *a, const void *b) {
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return (x > y) - (x < y);
}

typedef struct { float d; int64_t pos; } ooc_hit;
static int ooc_hit_cmp(const void *a, const void *b) {
    const ooc_hit *x = (const ooc_hit *)a, *y = (const ooc_hit *)b;
    if (x->d < y->d) return -1;
    if (x->d > y->d) return 1;
    return (x->pos > y->pos) - (x->pos < y->pos);
}

/* which rows of an out-of-core table one query keeps: whichever of the three is given, and a finite distance always */
typedef struct {
    const double *radius;              /* distance <= *radius */
    int has_set;                       /* the rowid is one of the n_ids SORTED ids */
    const int64_t *ids;
    int64_t n_ids;
    const double *after_dist;          /* behind the cursor (*after_dist, after_rowid): a larger distance, or an equal one and a larger rowid */
    int64_t after_rowid;
} ooc_keep;

/* query q against a table that does not fit the device: every distance through the slab path (k = 0), filtered, sorted by (distance,
 * scan position) and cut to `most` rows (<= 0: no cut) here - correct, not fast (INTEGRATION.md).  out_ids / out_dist: sqlite3_malloc'd
 * (*held rows), the caller frees them */
static int scan_ooc_query(scan_call *s, int q, const ooc_keep *keep, int64_t most, int64_t **out_ids, double **out_dist, int64_t *held) {
    scan_vtab *vt = s->vt;
    table_ctx *t = s->t;
    const uint8_t *one = s->scan_queries + q * s->qstep;
    float *all_dist = NULL;
    int64_t *all_ids = NULL, n = 0, m = 0;
    ooc_hit *hits = NULL;
    int got = 0;
    *out_ids = NULL; *out_dist = NULL; *held = 0;
    sqlite3_free(s->err); s->err = NULL;
    int rc = s->quantized ? ooc_scan_quant(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &s->err)
                          : ooc_scan_full(vt->db, t, one, 0, NULL, NULL, &got, &all_dist, &all_ids, &n, &s->err);
    if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", s->fname, s->err ? s->err : "scan failed"); goto done; }
    hits = (ooc_hit *)sqlite3_malloc64((sqlite3_uint64)(n > 0 ? n : 1) * sizeof(ooc_hit));
    if (!hits) { rc = SQLITE_NOMEM; goto done; }
    for (int64_t i = 0; i < n; ++i) {
        const double d = (double)all_dist[i];
        if (!(all_dist[i] < INFINITY)) continue;                                         /* NaN / +Inf never enter */
        if (keep->radius && !(d <= *keep->radius)) continue;
        if (keep->has_set && (keep->n_ids == 0 || !bsearch(&all_ids[i], keep->ids, (size_t)keep->n_ids, sizeof(int64_t), i64_cmp))) continue;
        if (keep->after_dist && !(d > *keep->after_dist || (d == *keep->after_dist && all_ids[i] > keep->after_rowid))) continue;
        hits[m].d = all_dist[i]; hits[m].pos = i; ++m;
    }
    qsort(hits, (size_t)m, sizeof(ooc_hit), ooc_hit_cmp);
    if (most > 0 && most < m) m = most;
    *out_ids = (int64_t *)sqlite3_malloc64((sqlite3_uint64)(m > 0 ? m : 1) * sizeof(int64_t));
    *out_dist = (double *)sqlite3_malloc64((sqlite3_uint64)(m > 0 ? m : 1) * sizeof(double));
    if (!*out_ids || !*out_dist) { rc = SQLITE_NOMEM; goto done; }
    for (int64_t i = 0; i < m; ++i) { (*out_ids)[i] = all_ids[hits[i].pos]; (*out_dist)[i] = (double)hits[i].d; }
    *held = m;
done:
    sqlite3_free(hits);
    sqlite3_free(all_dist);
    sqlite3_free(all_ids);
    return rc;
}

/* ... for every query of a top-k call, into its scan_topk_buffers (k slots per query) */
static int scan_ooc_topk(scan_call *s, int q, const ooc_keep *keep, int k) {
    int64_t *ids = NULL, held = 0;
    double *dist = NULL;
    int rc = scan_ooc_query(s, q, keep, k, &ids, &dist, &held);
    if (rc == SQLITE_OK) {
        memcpy(s->ids + (int64_t)q * k, ids, (size_t)held * sizeof(int64_t));
        memcpy(s->dist + (int64_t)q * k, dist, (size_t)held * sizeof(double));
        s->counts[q] = (int)held;
    }
    sqlite3_free(ids);
    sqlite3_free(dist);
    return rc;
}

/* ------------------------------------------------------------------------------------------------ range rows into the cursor */

/* the engine's fetch entry points of a range scan's result, single and batch form */
typedef int (*within_fetch_fn)(const vg_shards *, int64_t, int64_t, int64_t *, double *);
typedef int (*bwithin_fetch_fn)(const vg_shards *, int, int64_t, int64_t, int64_t *, double *);

/* room for `more` further rows in the cursor's three arrays (they hold stream_n rows, s->cap allocated) */
static int scan_rows_reserve(scan_call *s, int64_t more) {
    scan_cursor *c = s->c;
    const int64_t need = c->stream_n + more;
    if (need <= s->cap && c->rowids) return SQLITE_OK;
    int64_t ncap = s->cap ? s->cap : 64;
    while (ncap < need) ncap *= 2;
    int64_t *ids = (int64_t *)sqlite3_realloc64(c->rowids, (sqlite3_uint64)ncap * sizeof(int64_t));
    if (ids) c->rowids = ids;
    double *dist = (double *)sqlite3_realloc64(c->distance, (sqlite3_uint64)ncap * sizeof(double));
    if (dist) c->distance = dist;
    int *qn = (int *)sqlite3_realloc64(c->query_no, (sqlite3_uint64)ncap * sizeof(int));
    if (qn) c->query_no = qn;
    if (!ids || !dist || !qn) return SQLITE_NOMEM;
    s->cap = ncap;
    return SQLITE_OK;
}

/* the cursor gives up the rows of its previous call */
static void scan_rows_clear(scan_call *s) {
    scan_cursor *c = s->c;
    sqlite3_free(c->rowids); c->rowids = NULL;
    sqlite3_free(c->distance); c->distance = NULL;
    sqlite3_free(c->query_no); c->query_no = NULL;
    c->stream_n = 0;
    s->cap = 0;
}

/* INSIDE the lock, behind a range scan: per query, the held[q] rows the staged copy holds go behind the cursor's stream_n rows, stamped
 * with their query number (fetch: the single form's entry point, bfetch: the batch form's - one of them) */
static int scan_rows_fetch(scan_call *s, const int64_t *held, within_fetch_fn fetch, bwithin_fetch_fn bfetch) {
    scan_cursor *c = s->c;
    int64_t total = 0;
    for (int q = 0; q < s->nq; ++q) total += held[q];
    int rc = scan_rows_reserve(s, total > 0 ? total : 1);
    if (rc != SQLITE_OK) return rc;
    for (int q = 0; q < s->nq; ++q) {
        if (held[q] > 0 && (bfetch ? bfetch(s->corpus, q, 0, held[q], c->rowids + c->stream_n, c->distance + c->stream_n)
                                   : fetch(s->corpus, 0, held[q], c->rowids + c->stream_n, c->distance + c->stream_n)) != VG_OK)
            return vtab_error(&s->vt->base, "%s: %s", s->fname, gpu_error());
        for (int64_t i = 0; i < held[q]; ++i) c->query_no[c->stream_n + i] = q;
        c->stream_n += held[q];
    }
    return SQLITE_OK;
}

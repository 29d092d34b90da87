/* vext_range.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * range scans: every row whose distance is <= a radius, ordered by (distance, scan position) -
 *     vector_full_scan_within / vector_quantize_scan_within(table, column, vector, radius [, limit])                          -> (id, distance)
 *     vector_full_scan_within_filtered / vector_quantize_scan_within_filtered(table, column, vector, radius, filter [, limit]) -> (id, distance)
 *     vector_full_scan_batch_within / vector_quantize_scan_batch_within(table, column, queries, radius [, limit])             -> (query, id, distance)
 *     vector_full_scan_batch_within_filtered / vector_quantize_scan_batch_within_filtered(table, column, queries, radius, filter [, limit])
 * The reference's form of the question is "... FROM vector_full_scan_stream(...) WHERE distance <= ? [AND id IN (<filter>)]", N rows
 * stepped to keep a handful.  `queries` is the batch functions' argument (a BLOB of nq * dim elements or a JSON array of arrays), and
 * the rows come by query number (0-based) first; `radius` is a REAL / INTEGER - in the batch forms shared by all queries, or a JSON
 * array of exactly nq numbers; `filter` is the filtered functions' argument (vext_topk.inc: ONE read-only SELECT yielding rowids, or a
 * BLOB of packed int64 rowids; NULL is refused): only the rows it names are looked at; `limit` is per query.  Each query's rows of a
 * batch form are what the single form returns for it and its radius.
 * Staging, locks, tracked changes and freshness are vector_full_scan's (scan_stage); the compare-and-compact runs in the engine's scan
 * kernels, which share every row load between 4 (2) queries of a batch.  The row mask and the scan's result are state of the staged copy,
 * which several connections may share: mask, scan and fetch run inside ONE hold of the lock.  An out-of-core table answers query by
 * query through scan_ooc_query.  A single form is a batch of one that calls the engine's single entry points.
 */

SCAN_CONNECT(within_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, radius hidden, lim hidden);")
SCAN_CONNECT(wmasked_connect, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, radius hidden, filter hidden, lim hidden);")
SCAN_CONNECT(bwithin_connect, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, radius hidden, lim hidden);")
SCAN_CONNECT(bwmasked_connect, "CREATE TABLE x(query, id, distance, tbl hidden, col hidden, queries hidden, radius hidden, filter hidden, lim hidden);")

/* the engine's range-scan entry points, plain and masked alike (the fetch ones: vext_scanform.inc) */
typedef int (*masked_set_fn)(vg_shards *, const int64_t *, int64_t, int64_t *);
typedef int (*within_scan_fn)(vg_shards *, int, const void *, double, int64_t, int64_t *, int64_t *);
typedef int (*bwithin_scan_fn)(vg_shards *, int, const void *, int, const double *, int64_t, int64_t *, int64_t *);

static int masked_filter_arg(scan_vtab *vt, const char *fname, sqlite3_value *arg, int64_t **out_ids, int64_t *out_n);      /* vext_topk.inc */

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

/* One xFilter for the four forms: (table, column, vector | queries, radius [, filter] [, limit]) */
static int range_filter_form(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized, int batch, int masked) {
    static const arg_spec specs[2][2] = {
        {{4, "%s expects 4 or 5 arguments, but %d were provided.", {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_NUMBER, ARG_INTEGER}},
         {5, "%s expects 5 or 6 arguments, but %d were provided.", {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_NUMBER, ARG_FILTER, ARG_INTEGER}}},
        {{4, "%s expects 4 or 5 arguments, but %d were provided.", {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_NUMBER_OR_JSON, ARG_INTEGER}},
         {5, "%s expects 5 or 6 arguments, but %d were provided.", {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_NUMBER_OR_JSON, ARG_FILTER, ARG_INTEGER}}}};
    const arg_spec *spec = &specs[batch][masked];
    scan_call s;
    scan_begin(&s, cur, fname, quantized, 0);
    scan_vtab *vt = s.vt;
    double *radii_owned = NULL, radius = 0.0;
    int64_t *filter_ids = NULL, *matches = NULL, *held = NULL, filter_n = 0;
    int rc = scan_check_args(vt, fname, spec, argc, argv);
    if (rc != SQLITE_OK) return rc;
    if ((rc = scan_lookup(&s, argv)) != SQLITE_OK) goto out;
    table_ctx *t = s.t;
    if (batch && sqlite3_value_type(argv[2]) == SQLITE_BLOB) {
        const int64_t bytes = sqlite3_value_bytes(argv[2]), qrow = (int64_t)t->opt.v_dim * elem_size(t->opt.v_type);
        if (bytes == 0 || bytes % qrow != 0) {
            rc = vtab_error(&vt->base, "%s: query vector has %lld bytes, expected a multiple of %lld (dimension %d).", fname, (long long)bytes, (long long)qrow, t->opt.v_dim);
            goto out;
        }
    }
    if ((rc = scan_open(&s, argv, batch, fname)) != SQLITE_OK) goto out;

    const int has_limit = argc == spec->n + 1;
    const int64_t limit = has_limit ? (int64_t)sqlite3_value_int64(argv[spec->n]) : -1;    /* -1: none */
    if (has_limit && limit < 0) { rc = vtab_error(&vt->base, "%s: limit must not be negative.", fname); goto out; }
    if (batch) {
        if ((rc = bwithin_radius_arg(vt, fname, argv[3], s.nq, &radii_owned)) != SQLITE_OK) goto out;
    } else {
        radius = sqlite3_value_double(argv[3]);
        if (!masked && has_limit && limit == 0) goto out;                                /* (the plain single form looks at limit = 0 first) */
        if (radius != radius) { rc = vtab_error(&vt->base, "%s: radius cannot be NaN.", fname); goto out; }
    }
    if ((has_limit && limit == 0) || s.nq == 0) goto out;                                /* no rows, no device (decided here, like k = 0) */
    const double *radii = batch ? radii_owned : &radius;

    /* the allowed rowids: before anything is staged - a refused filter runs nothing */
    if (masked && (rc = masked_filter_arg(vt, fname, argv[4], &filter_ids, &filter_n)) != SQLITE_OK) goto out;

    /* an engine without the entry points still loads, the functions then say so */
    const char *names[3];
    void *fn[3];
    int nfn = 0;
    if (masked) names[nfn++] = "vg_shards_set_mask_rowids";
    names[nfn++] = batch ? (masked ? "vg_shards_scan_within_batch_masked" : "vg_shards_scan_within_batch")
                         : (masked ? "vg_shards_scan_within_masked" : "vg_shards_scan_within");
    names[nfn++] = batch ? "vg_shards_scan_within_batch_fetch" : "vg_shards_scan_within_fetch";
    const char *missing = scan_resolve(&s, names, fn, nfn);
    if (missing) {
        rc = masked ? vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (masked range scans need a newer libvectorgpu.so).", fname, missing)
           : batch  ? vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (batch range scans need a newer libvectorgpu.so).", fname, missing)
                    : vtab_error(&vt->base, "%s: the GPU engine lacks symbol %s (range scans need a newer libvectorgpu.so).", fname, missing);
        goto out;
    }
    if ((rc = scan_stage(&s)) != SQLITE_OK) goto out;

    scan_rows_clear(&s);
    if (s.ooc) {
        if (filter_n > 1) qsort(filter_ids, (size_t)filter_n, sizeof(int64_t), i64_cmp);
        if ((rc = scan_rows_reserve(&s, 1)) != SQLITE_OK) goto out;
        for (int q = 0; q < s.nq; ++q) {                 /* each query reads the table again */
            const ooc_keep keep = {&radii[q], masked, filter_ids, filter_n, NULL, 0};
            int64_t *ids = NULL, n = 0;
            double *dist = NULL;
            rc = scan_ooc_query(&s, q, &keep, limit, &ids, &dist, &n);
            if (rc == SQLITE_OK) rc = scan_rows_reserve(&s, n);
            for (int64_t i = 0; rc == SQLITE_OK && i < n; ++i, ++s.c->stream_n) {
                s.c->rowids[s.c->stream_n] = ids[i];
                s.c->distance[s.c->stream_n] = dist[i];
                s.c->query_no[s.c->stream_n] = q;
            }
            sqlite3_free(ids);
            sqlite3_free(dist);
            if (rc != SQLITE_OK) goto out;
        }
        goto out;
    }

    matches = (int64_t *)sqlite3_malloc64((sqlite3_uint64)s.nq * sizeof(int64_t));
    held = (int64_t *)sqlite3_malloc64((sqlite3_uint64)s.nq * sizeof(int64_t));
    if (!matches || !held) { rc = SQLITE_NOMEM; goto out; }
    scan_lock(&s);
    {
        int64_t allowed = 0;
        const int64_t lim = limit > 0 ? limit : 0;
        void *scan = fn[nfn - 2];
        if ((masked && ((masked_set_fn)fn[0])(s.corpus, filter_ids, filter_n, &allowed) != VG_OK) ||
            (batch ? ((bwithin_scan_fn)scan)(s.corpus, t->opt.v_distance, s.scan_queries, s.nq, radii, lim, matches, held)
                   : ((within_scan_fn)scan)(s.corpus, t->opt.v_distance, s.scan_queries, radii[0], lim, matches, held)) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        rc = scan_rows_fetch(&s, held, batch ? NULL : (within_fetch_fn)fn[nfn - 1], batch ? (bwithin_fetch_fn)fn[nfn - 1] : NULL);
    }
out:
    sqlite3_free(radii_owned);
    sqlite3_free(filter_ids);
    sqlite3_free(matches);
    sqlite3_free(held);
    return scan_close(&s, rc);
}

static int within_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return range_filter_form(cur, argc, argv, fname, quantized, 0, 0); }
static int wmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return range_filter_form(cur, argc, argv, fname, quantized, 0, 1); }
static int bwithin_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return range_filter_form(cur, argc, argv, fname, quantized, 1, 0); }
static int bwmasked_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) { return range_filter_form(cur, argc, argv, fname, quantized, 1, 1); }

SCAN_FORM(within, "_within", within_filter_common, within_connect, single_best_index, within_next, within_eof, within_column, within_rowid);
SCAN_FORM(wmasked, "_within_filtered", wmasked_filter_common, wmasked_connect, single_best_index, within_next, within_eof, within_column, within_rowid);
SCAN_FORM(bwithin, "_batch_within", bwithin_filter_common, bwithin_connect, brange_best_index, within_next, within_eof, bwithin_column, bwithin_rowid);
SCAN_FORM(bwmasked, "_batch_within_filtered", bwmasked_filter_common, bwmasked_connect, brange_best_index, within_next, within_eof, bwithin_column, bwithin_rowid);

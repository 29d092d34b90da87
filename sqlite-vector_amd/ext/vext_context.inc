/* vext_context.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * per-connection context: options of a (table, column), its HBM-resident corpora, error helpers
 */
/* ------------------------------------------------------------------------------------------------ context */

typedef struct {
    int v_type;                 /* VG_TYPE_* (same numbering as the reference's vector_type) */
    int v_dim;
    int v_normalized;
    int v_distance;             /* VG_DIST_* */
    int q_type;                 /* VG_QUANT_* */
    uint64_t max_memory;
    char gpu_devices[64];       /* additions (ignored by the reference): where the corpus lives */
    int64_t gpu_shard_rows;
    int tie_order;              /* -1 = default, VG_TIE_POSITION, VG_TIE_REFERENCE (option tie_order=position|reference) */
    int scan_filter;            /* -1 = default, 0 / 1 (option scan_filter=0|1): f32 / f16 / bf16 scans through a shadow-copy filter */
    int track_changes;          /* -1 = default (VECTORGPU_TRACK_CHANGES, else off), 0 / 1 (option track_changes=0|1): row-granular
                                   freshness for UPDATE / DELETE through sqlite3_update_hook - see on_row_change() */
} vec_options;

/* Result order among EQUAL distances.  tie_order=reference is the reference's own result, rowid for rowid - its slot algorithm
 * (sqlite-vector.c:2022-2069, 2102-2106) is history dependent among ties.  It costs what tie_order=position costs unless the k + 1
 * best distances of a query hold a tie (then a host replay over the few rows that can enter the slots, vg_reforder.hip), so it is
 * the DEFAULT wherever ties are routine: integer element types - every vector_quantize_scan, and full scans of INT8 / UINT8
 * columns (north_star: "bit-exact rowid/top-k ordering for int8/uint8").  Float columns default to (distance, scan position):
 * their distances differ from the reference's in the last bits anyway (f32 <= 1e-5), exact ties are duplicates.
 * Explicit: the tie_order= option, else the VECTORGPU_TIE_ORDER environment variable. */
static int tie_order_for(const vec_options *o, int vtype) {
    if (o->tie_order >= 0) return o->tie_order;
    const char *e = getenv("VECTORGPU_TIE_ORDER");
    if (e && *e) return !strcasecmp(e, "reference") ? VG_TIE_REFERENCE : VG_TIE_POSITION;
    return (vtype == VG_TYPE_U8 || vtype == VG_TYPE_I8) ? VG_TIE_REFERENCE : VG_TIE_POSITION;
}

static int corpus_open_spec(const vec_options *o, int vtype, int dim, vg_shards **out) {
    int rc = corpus_open_devices(o->gpu_devices, o->gpu_shard_rows, vtype, dim, out);
    if (rc != VG_OK) return rc;
    if ((rc = G.corpus_set_tie_order(*out, tie_order_for(o, vtype))) != VG_OK ||
        (rc = G.corpus_set_scan_filter(*out, o->scan_filter)) != VG_OK) {
        G.corpus_destroy(*out);
        *out = NULL;
    }
    return rc;
}

typedef struct {
    char *t_name, *c_name, *pk_name;
    vec_options opt;
    float scale, offset;        /* quantization parameters (persisted as qscale / qoffset) */

    /* HBM-resident state owned by this (table, column) */
    vg_shards *full;            /* raw vectors for vector_full_scan[_stream] */
    int64_t full_data_version;  /* staleness stamps: PRAGMA data_version + sqlite3_total_changes() + PRAGMA schema_version */
    int64_t full_changes;
    int64_t full_schema;
    int64_t full_table_rows;    /* COUNT(*) of the table when it was staged (NULL vectors included) and its largest key: */
    int64_t full_max_pk;        /*   what the append-only check of stage_full() compares against */
    int full_have_pk;
    int full_in_txn;            /* staged inside an open transaction: a ROLLBACK leaves both stamps unchanged */
    int full_validated;         /* set when stage_full() (re)validated `full` during the current vector_quantize call */
    int full_prestaged;         /* vector_quantize staged `full` in front of its transaction (where the parallel readers can serve it) */
    /* change tracking (track_changes=1): rowids of this table touched since `full` was last brought up to date */
    int64_t *touched;
    int n_touched, cap_touched, touched_overflow;
    int64_t hook_seen;          /* vec_context.hook_events at that moment; -1: `full` was staged without the hook in place */
    vg_shards *quant;           /* quantized vectors for vector_quantize_scan[_stream] */
    int quant_preloaded;        /* explicit vector_quantize_preload() (kept until cleanup / re-quantize) */
    int64_t quant_data_version;
    int64_t quant_changes;
    int64_t quant_schema;
    int quant_in_txn;
    /* out of core: the table (its quantized records) does not fit the device(s) - VECTORGPU_HBM_LIMIT or the free memory found - and
     * every scan walks the rows again, slab by slab (the reference walks them for every scan anyway); see ooc_plan() */
    /* one staged copy per process (vext_shared.inc): set while `full` / `quant` is the registry's copy - immutable, scanned under its mutex */
    shared_corpus *full_sh, *quant_sh;
    int full_ooc, quant_ooc;
    int64_t full_slab_rows, quant_slab_rows;
    int ooc_device;
    /* the HOST-RESIDENT tier of an out-of-core table (round 6): its rows and keys once in pinned host memory (vg_host_alloc), every scan
     * streams them over the host link instead of walking the table through sqlite3_step again; same stamps as a device copy */
    uint8_t *host_rows;
    int64_t *host_ids;
    int64_t host_n, host_cap;
    int64_t host_data_version, host_changes, host_schema;
    int host_in_txn, host_off;                  /* host_off: tried and refused (limit, allocation, more rows than the bound) - until the stamps move */
    int host_sink;                              /* the staging loop's rows go to the host copy (vext_staging.inc: stage_rows_put) */
    /* labeled scans (vext_labeled.inc), [0] the raw copy, [1] the quantized one: which label column this connection last set on the
     * staged copy, on which handle, under which stamps (db_stamps; in_txn: read inside an open transaction - never reused), and the
     * generation it left on a shared copy (another connection's set_labels moves it) */
    char *lab_col[2];
    vg_shards *lab_corpus[2];
    int64_t lab_data_version[2], lab_changes[2], lab_schema[2];
    int lab_in_txn[2];
    uint64_t lab_gen[2];
} table_ctx;

typedef struct {
    table_ctx tables[MAX_TABLES];
    int count;
    int hook_installed;         /* sqlite3_update_hook(db, on_row_change, this) was called for this connection */
    int64_t hook_events;        /* row changes it has reported so far (every table, every attached database) */
} vec_context;

static int elem_size(int t) {
    switch (t) {
        case VG_TYPE_F32: return 4;
        case VG_TYPE_F16: case VG_TYPE_BF16: return 2;
        case VG_TYPE_U8: case VG_TYPE_I8: return 1;
    }
    return 0;
}

static const char *type_name(int t) {
    switch (t) {
        case VG_TYPE_F32: return "FLOAT32"; case VG_TYPE_F16: return "FLOAT16"; case VG_TYPE_BF16: return "FLOATB16";
        case VG_TYPE_U8: return "UINT8"; case VG_TYPE_I8: return "INT8";
    }
    return "N/A";
}

static int type_from_name(const char *s) {
    if (!strcasecmp(s, "FLOAT32")) return VG_TYPE_F32;
    if (!strcasecmp(s, "FLOAT16")) return VG_TYPE_F16;
    if (!strcasecmp(s, "FLOATB16")) return VG_TYPE_BF16;
    if (!strcasecmp(s, "UINT8")) return VG_TYPE_U8;
    if (!strcasecmp(s, "INT8")) return VG_TYPE_I8;
    return 0;
}

static int distance_from_name(const char *s) {
    if (!strcasecmp(s, "L2") || !strcasecmp(s, "EUCLIDEAN")) return VG_DIST_L2;
    if (!strcasecmp(s, "SQUARED_L2")) return VG_DIST_SQUARED_L2;
    if (!strcasecmp(s, "COSINE")) return VG_DIST_COSINE;
    if (!strcasecmp(s, "DOT") || !strcasecmp(s, "INNER")) return VG_DIST_DOT;
    if (!strcasecmp(s, "L1") || !strcasecmp(s, "MANHATTAN")) return VG_DIST_L1;
    return 0;
}

static const char *sql_type_name(int t) {
    switch (t) {
        case SQLITE_TEXT: return "TEXT"; case SQLITE_INTEGER: return "INTEGER";
        case SQLITE_FLOAT: return "REAL"; case SQLITE_BLOB: return "BLOB";
    }
    return "N/A";
}

static char *dup_str(const char *s) {
    if (!s) return NULL;
    size_t n = strlen(s) + 1;
    char *r = (char *)sqlite3_malloc((int)n);
    if (r) memcpy(r, s, n);
    return r;
}

/* the message of the last ctx_error() on this thread: callers that post-process a failure (vector_quantize rolls back
 * and would otherwise report sqlite3_errmsg() = "not an error" for a failure that did not come from SQLite) keep it */
static __thread char last_ctx_error[1024];

static void ctx_error(sqlite3_context *ctx, int rc, const char *fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    strncpy(last_ctx_error, buf, sizeof(last_ctx_error) - 1);
    last_ctx_error[sizeof(last_ctx_error) - 1] = 0;
    sqlite3_result_error(ctx, buf, -1);
    sqlite3_result_error_code(ctx, rc);
}

static int vtab_error(sqlite3_vtab *vt, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    if (vt->zErrMsg) sqlite3_free(vt->zErrMsg);
    vt->zErrMsg = sqlite3_vmprintf(fmt, ap);
    va_end(ap);
    return SQLITE_ERROR;
}

/* this connection lets go of its copy: its own one is destroyed, the registry's loses a reference */
static void host_release(table_ctx *t) {
    if (t->host_rows && G.host_free) G.host_free(t->host_rows);
    if (t->host_ids && G.host_free) G.host_free(t->host_ids);
    t->host_rows = NULL; t->host_ids = NULL; t->host_n = 0; t->host_cap = 0; t->host_sink = 0;
}
static void full_release(table_ctx *t) {
    if (t->full_sh) shared_unref(t->full_sh);
    else if (t->full) G.corpus_destroy(t->full);
    t->full_sh = NULL;
    t->full = NULL;
}
static void quant_release(table_ctx *t) {
    if (t->quant_sh) shared_unref(t->quant_sh);
    else if (t->quant) G.corpus_destroy(t->quant);
    t->quant_sh = NULL;
    t->quant = NULL;
}
/* before `full` is CHANGED (restaged in place, appended to, patched): the only holder keeps the corpus; anyone else gets a CLONE of it
 * (a device-to-device copy: milliseconds per 10 GB, against a pass over the table) so that the row-granular update paths - the rows this
 * connection appended, the rows its update hook logged - still apply; no room for a second copy on the device: start afresh */
static void full_make_private(table_ctx *t) {
    if (!t->full_sh) return;
    shared_corpus *e = t->full_sh;
    t->full_sh = NULL;
    t->full = shared_take_private_or_keep(e);
    if (t->full) return;                                        /* (the only holder: the entry is gone, the corpus is ours) */
    vg_shards *copy = NULL;                                     /* (others hold it too: our reference is kept while the rows are copied) */
    pthread_mutex_lock(&e->mu);                                 /* (no scan of the source in the meantime) */
    const int rc = G.corpus_clone(e->corpus, &copy);
    pthread_mutex_unlock(&e->mu);
    shared_unref(e);
    if (rc == VG_OK) t->full = copy;
}
/* scans of a shared copy are serialized (the engine's handles are not re-entrant) */
static void full_lock(table_ctx *t) { if (t->full_sh) pthread_mutex_lock(&t->full_sh->mu); }
static void full_unlock(table_ctx *t) { if (t->full_sh) pthread_mutex_unlock(&t->full_sh->mu); }
static void quant_lock(table_ctx *t) { if (t->quant_sh) pthread_mutex_lock(&t->quant_sh->mu); }
static void quant_unlock(table_ctx *t) { if (t->quant_sh) pthread_mutex_unlock(&t->quant_sh->mu); }

static void table_release_gpu(table_ctx *t) {
    host_release(t);
    full_release(t);
    quant_release(t);
    t->quant_preloaded = 0;
}

static void context_free(void *p) {
    vec_context *c = (vec_context *)p;
    if (!c) return;
    for (int i = 0; i < c->count; ++i) {
        table_release_gpu(&c->tables[i]);
        sqlite3_free(c->tables[i].t_name);
        sqlite3_free(c->tables[i].c_name);
        sqlite3_free(c->tables[i].pk_name);
        sqlite3_free(c->tables[i].touched);
        sqlite3_free(c->tables[i].lab_col[0]);
        sqlite3_free(c->tables[i].lab_col[1]);
    }
    sqlite3_free(c);
}

static table_ctx *context_lookup(vec_context *c, const char *tbl, const char *col) {
    if (!tbl || !col) return NULL;
    for (int i = 0; i < c->count; ++i) {
        table_ctx *t = &c->tables[i];
        if (t->t_name && t->c_name && !strcasecmp(t->t_name, tbl) && !strcasecmp(t->c_name, col)) return t;
    }
    return NULL;
}

/* vext_cursor.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * the vtab and the cursor every module shares, and the xNext / xEof / xColumn / xRowid of the four output layouts
 */
typedef struct {
    sqlite3_vtab base;
    sqlite3 *db;
    vec_context *ctx;
} scan_vtab;

typedef struct {
    sqlite3_vtab_cursor base;
    int streaming;
    /* materialised rows: row_count of them for the reference's layout and the batch top-k forms (32-bit counters), stream_n of them for
     * the added single forms and the batch range forms (64-bit counters: a radius may match every row of a large table) */
    int64_t *rowids;
    double *distance;
    int row_index, row_count;
    int *query_no;                     /* batch TVFs: which query of the batch each output row answers */
    /* streaming: all N distances computed by ONE kernel launch, paged out row by row */
    float *all_dist;
    int64_t *all_rowids;               /* the cursor's own snapshot: the corpus may be re-staged / destroyed while it is stepped */
    int64_t stream_pos, stream_n;
} scan_cursor;

static int tvf_disconnect(sqlite3_vtab *v) { sqlite3_free(v); return SQLITE_OK; }

static int tvf_open(sqlite3_vtab *v, sqlite3_vtab_cursor **out) {
    scan_cursor *c = (scan_cursor *)sqlite3_malloc(sizeof(scan_cursor));
    if (!c) return SQLITE_NOMEM;
    memset(c, 0, sizeof(*c));
    *out = &c->base;
    return SQLITE_OK;
}

static int tvf_close(sqlite3_vtab_cursor *cur) {
    scan_cursor *c = (scan_cursor *)cur;
    sqlite3_free(c->rowids);
    sqlite3_free(c->distance);
    sqlite3_free(c->all_dist);
    sqlite3_free(c->all_rowids);
    sqlite3_free(c->query_no);
    sqlite3_free(c);
    return SQLITE_OK;
}

/* ---- the reference's layout (tbl, vector, k, memidx hidden; id, distance [, query]) */
static int tvf_next(sqlite3_vtab_cursor *cur) {
    scan_cursor *c = (scan_cursor *)cur;
    if (c->streaming) c->stream_pos++; else c->row_index++;
    return SQLITE_OK;
}

static int tvf_eof(sqlite3_vtab_cursor *cur) {
    scan_cursor *c = (scan_cursor *)cur;
    return c->streaming ? (c->stream_pos >= c->stream_n) : (c->row_index >= c->row_count);
}

static sqlite3_int64 cursor_rowid(scan_cursor *c) {
    return c->streaming ? (sqlite3_int64)c->all_rowids[c->stream_pos] : (sqlite3_int64)c->rowids[c->row_index];
}

static int tvf_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == COL_ID) sqlite3_result_int64(ctx, cursor_rowid(c));
    else if (col == COL_DISTANCE) sqlite3_result_double(ctx, c->streaming ? (double)c->all_dist[c->stream_pos] : c->distance[c->row_index]);
    else if (col == COL_QUERY && c->query_no) sqlite3_result_int(ctx, c->query_no[c->row_index]);
    return SQLITE_OK;
}

static int tvf_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = cursor_rowid((scan_cursor *)cur);
    return SQLITE_OK;
}

/* ---- the added single forms: (id, distance, hidden arguments ...), stream_n rows */
enum { WCOL_ID = 0, WCOL_DISTANCE = 1, WCOL_TBL = 2, WCOL_LAST = 8 };      /* (WCOL_LAST: the last hidden column of the longest form) */

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

/* ---- the added batch forms: (query, id, distance, hidden arguments ...); the range forms step stream_n rows (within_next / within_eof),
 * the top-k forms row_count rows (tvf_next / tvf_eof / tvf_rowid) */
enum { BCOL_QUERY = 0, BCOL_ID = 1, BCOL_DISTANCE = 2, BCOL_TBL = 3, BCOL_LAST = 8 };

static int bwithin_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == BCOL_QUERY) sqlite3_result_int(ctx, c->query_no[c->stream_pos]);
    else if (col == BCOL_ID) sqlite3_result_int64(ctx, (sqlite3_int64)c->rowids[c->stream_pos]);
    else if (col == BCOL_DISTANCE) sqlite3_result_double(ctx, c->distance[c->stream_pos]);
    return SQLITE_OK;
}
static int bwithin_rowid(sqlite3_vtab_cursor *cur, sqlite3_int64 *out) {
    *out = (sqlite3_int64)((scan_cursor *)cur)->stream_pos;
    return SQLITE_OK;
}
static int bmasked_column(sqlite3_vtab_cursor *cur, sqlite3_context *ctx, int col) {
    scan_cursor *c = (scan_cursor *)cur;
    if (col == BCOL_QUERY) sqlite3_result_int(ctx, c->query_no[c->row_index]);
    else if (col == BCOL_ID) sqlite3_result_int64(ctx, (sqlite3_int64)c->rowids[c->row_index]);
    else if (col == BCOL_DISTANCE) sqlite3_result_double(ctx, c->distance[c->row_index]);
    return SQLITE_OK;
}

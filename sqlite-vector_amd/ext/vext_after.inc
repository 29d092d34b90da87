/* vext_after.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * paged scans ("search after"): the next k rows behind a (distance, rowid) cursor, ordered by (distance, scan position) -
 *     vector_full_scan_after / vector_quantize_scan_after(table, column, vector, k, after_distance, after_rowid)
 *     vector_full_scan_filtered_after / vector_quantize_scan_filtered_after(table, column, vector, k, filter, after_distance, after_rowid)
 * -> (id, distance).  The cursor is the distance and id of the previous page's last row; both NULL = the first page, exactly one
 * NULL, a cursor that is no number and k outside 1..64 are errors.  A row is behind the cursor when its distance is larger, or equal
 * with a larger rowid: pages never repeat or skip a row, also inside a run of equal distances, and a page taken after the cursor's row
 * was deleted continues where it should.  It answers "... ORDER BY distance, id LIMIT k OFFSET m" without the top-(m + k) scan.
 * Everything but the argument list and the engine call is the masked functions' (vext_masked.inc: masked_filter_form - staging, the
 * lock held across set-mask-and-scan, tracked changes, the filter argument, the out-of-core answer); cursor, columns and next / eof
 * are the within functions' (vext_within.inc).
 */
enum { ACOL_LAST = 7, FACOL_LAST = 8 };          /* the last hidden argument column: after_rowid */

static int after_connect_sql(sqlite3 *db, void *aux, sqlite3_vtab **out, const char *decl) {
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
static int after_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    return after_connect_sql(db, aux, out, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, after_distance hidden, after_rowid hidden);");
}
static int fafter_connect(sqlite3 *db, void *aux, int argc, const char *const *argv, sqlite3_vtab **out, char **err) {
    return after_connect_sql(db, aux, out, "CREATE TABLE x(id, distance, tbl hidden, col hidden, vector hidden, k hidden, filter hidden, after_distance hidden, after_rowid hidden);");
}

/* the within functions' index plan with every hidden argument column up to `last` handed to xFilter in order */
static int after_plan(sqlite3_vtab *v, sqlite3_index_info *info, int last) {
    int rc = within_best_index(v, info);
    for (int i = 0; rc == SQLITE_OK && i < info->nConstraint; ++i) {
        const struct sqlite3_index_constraint *c = &info->aConstraint[i];
        if (!c->usable || c->op != SQLITE_INDEX_CONSTRAINT_EQ || c->iColumn <= WCOL_LIMIT || c->iColumn > last) continue;
        info->aConstraintUsage[i].argvIndex = c->iColumn - WCOL_TBL + 1;
        info->aConstraintUsage[i].omit = 1;
    }
    return rc;
}
static int after_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return after_plan(v, info, ACOL_LAST); }
static int fafter_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return after_plan(v, info, FACOL_LAST); }

static int full_after_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_full_scan_after", 0, 0, 1); }
static int quant_after_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_quantize_scan_after", 1, 0, 1); }
static int full_fafter_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_full_scan_filtered_after", 0, 1, 1); }
static int quant_fafter_filter(sqlite3_vtab_cursor *c, int n, const char *s, int argc, sqlite3_value **argv) { return masked_filter_form(c, argc, argv, "vector_quantize_scan_filtered_after", 1, 1, 1); }

static sqlite3_module full_after_module = {0, 0, after_connect, after_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_after_filter,
                                           within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_after_module = {0, 0, after_connect, after_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_after_filter,
                                            within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module full_fafter_module = {0, 0, fafter_connect, fafter_best_index, tvf_disconnect, 0, tvf_open, tvf_close, full_fafter_filter,
                                            within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static sqlite3_module quant_fafter_module = {0, 0, fafter_connect, fafter_best_index, tvf_disconnect, 0, tvf_open, tvf_close, quant_fafter_filter,
                                             within_next, within_eof, within_column, within_rowid, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

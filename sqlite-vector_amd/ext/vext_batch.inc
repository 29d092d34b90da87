/* vext_batch.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * vector_full_scan_batch / vector_quantize_scan_batch
 */
/* ---- batched queries (SURVEY 8f-4; the reference has no multi-query entry point: its equivalent is nq separate
 * vector_full_scan statements).  vector_full_scan_batch(tbl, col, queries, k) / vector_quantize_scan_batch(...):
 *   queries  BLOB of nq * dim elements (query vectors back to back), or TEXT JSON array of arrays
 *   output   (query, id, distance): k rows per query, ordered by query number (0-based) then distance ascending
 * Each query's rows are what the single-query function returns for it; f32 DOT/COSINE batches run as one
 * matrix-core pass over the corpus (vg_scan_topk_batch), everything else as nq GPU scans. */

SCAN_CONNECT(batch_connect, "CREATE TABLE x(tbl hidden, vector hidden, k hidden, memidx hidden, id, distance, query);")

static int batch_best_index(sqlite3_vtab *v, sqlite3_index_info *info) { return plan_batch(info, 2, COL_TBL, COL_MEMIDX, COL_QUERY, COL_DISTANCE); }

static int batch_filter_common(sqlite3_vtab_cursor *cur, int argc, sqlite3_value **argv, const char *fname, int quantized) {
    static const arg_spec args = {4, NULL, {ARG_TEXT, ARG_TEXT, ARG_VECTOR, ARG_INTEGER}};
    scan_call s;
    scan_begin(&s, cur, fname, quantized, 0);
    scan_vtab *vt = s.vt;
    int rc = scan_check_args(vt, fname, &args, argc, argv);
    if (rc != SQLITE_OK) return rc;
    if ((rc = scan_open(&s, argv, 1, NULL)) != SQLITE_OK) goto out;
    table_ctx *t = s.t;
    const int k = sqlite3_value_int(argv[3]);
    if (k == 0 || s.nq == 0) { rc = (k == 0) ? SQLITE_DONE : SQLITE_OK; goto out; }
    if (k < 0) { rc = vtab_error(&vt->base, "%s: k must be positive.", fname); goto out; }
    if ((rc = scan_quant_table(&s, "vector_quantize_scan")) != SQLITE_OK) goto out;       /* (the reference's text, as in vext_tvf.inc) */
    if ((rc = scan_stage(&s)) != SQLITE_OK) goto out;

    const int64_t n = s.ooc ? (int64_t)k : G.corpus_rows(s.corpus);
    const int kk = (int)((int64_t)k < n ? (int64_t)k : (n > 0 ? n : 1));     /* never more than N rows per query */
    if ((rc = scan_topk_buffers(&s, kk)) != SQLITE_OK) goto out;
    if (s.ooc) {
        /* a table that does not fit the device: Q independent scans, each reading the table again - what Q calls of the reference's
         * vector_full_scan do (vext_staging.inc: ooc_plan) */
        for (int i = 0; i < s.nq; ++i) {
            const uint8_t *one = s.scan_queries + i * s.qstep;
            rc = quantized ? ooc_scan_quant(vt->db, t, one, kk, s.ids + (int64_t)i * kk, s.dist + (int64_t)i * kk, &s.counts[i], NULL, NULL, NULL, &s.err)
                           : ooc_scan_full(vt->db, t, one, kk, s.ids + (int64_t)i * kk, s.dist + (int64_t)i * kk, &s.counts[i], NULL, NULL, NULL, &s.err);
            if (rc != SQLITE_OK) { rc = vtab_error(&vt->base, "%s: %s", fname, s.err ? s.err : "scan failed"); goto out; }
        }
    } else {
        scan_lock(&s);
        if (G.scan_topk_batch(s.corpus, t->opt.v_distance, s.scan_queries, s.nq, kk, s.ids, s.dist, s.counts) != VG_OK) {
            rc = vtab_error(&vt->base, "%s: %s", fname, gpu_error());
            goto out;
        }
        scan_unlock(&s);
    }
    rc = batch_emit(s.c, s.nq, kk, s.ids, s.dist, s.counts);
out:
    return scan_close(&s, rc);
}

SCAN_FORM(batch, "_batch", batch_filter_common, batch_connect, batch_best_index, tvf_next, tvf_eof, tvf_column, tvf_rowid);

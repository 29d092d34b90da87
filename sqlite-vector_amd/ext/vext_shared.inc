/* vext_shared.inc - part of vector_ext.c (one translation unit: #include'd there, in order; every function is static).
 * ONE staged copy per process: a registry of device-resident corpora that the connections of a process share
 *
 * The reference keeps nothing resident for vector_full_scan and one malloc'd buffer per CONNECTION for a preloaded quantization
 * (sqlite-vector.c:1338-1404: the buffer hangs off the connection's table_context) - host memory is cheap enough for that.  Device
 * memory is not: eight connections of a server process over one 150 GB table must not hold eight copies.  So a staged corpus is
 * published here, keyed by WHAT IT IS A COPY OF, and the next connection that needs the same copy takes a reference instead of reading
 * the table again.
 *
 * Identity of a copy = (database file: path + device + inode, table, column, what it was built as: kind / element type / dimension /
 * device list / block size / tie order / filter option) + the database file's CHANGE COUNTER (bytes 24..27 of page 1) at the moment the
 * rows were read.  In rollback-journal mode every committing write transaction increments that counter and the file only changes
 * under an EXCLUSIVE lock, so a connection that holds a SHARED lock and reads counter c sees exactly the content every other
 * connection saw under the same c.  (PRAGMA data_version tells ONE connection that something changed; it cannot be compared across
 * connections - the counter can.)  Not shareable, and handled by the per-connection logic as before: in-memory and temporary
 * databases, WAL mode (the counter in the main file does not follow WAL commits), a connection inside a transaction (its own
 * uncommitted rows), a table shadowed by a TEMP table or living in an attached database, a file that was moved or deleted under the
 * connection.  VECTORGPU_SHARE=0 switches the registry off.
 *
 * A shared corpus is IMMUTABLE: the row-granular update paths (append-only restaging, tracked changes) first take it private - free of
 * charge for the only holder, a fresh copy otherwise - and publish the result under the new counter.  The engine's handles are not
 * re-entrant (working buffers, streams), so a scan over a shared corpus holds the entry's mutex; the device serialises the kernels of
 * one corpus anyway. */
#include <sys/stat.h>

typedef struct shared_corpus {
    char *key;
    uint32_t counter;
    vg_shards *corpus;
    int refs;
    pthread_mutex_t mu;                         /* one scan of this corpus at a time */
    int64_t table_rows, max_pk;                 /* the staging pass' watermark (vext_staging.inc) travels with the copy */
    int have_pk;
    uint64_t label_gen;                         /* labeled scans (vext_labeled.inc): which set_labels the copy's labels are from (under mu) */
    struct shared_corpus *next;
} shared_corpus;

static shared_corpus *g_shared;                                          /* the registry: a short list (entries = distinct live copies) */
static pthread_mutex_t g_shared_mu = PTHREAD_MUTEX_INITIALIZER;          /* guards the list and every refs field */
/* N connections that need the SAME copy at once stage it once: the first one to miss registers the (key, counter) it is about to stage in
 * g_inflight and reads the table WITHOUT any process-wide lock; the others wait on g_stage_cv and look again when a staging pass ends.
 * Connections after another table, another file or an already published copy never wait for it (round 5 held one mutex across the whole
 * pass: a 150 GB table stalled every first scan of the process for minutes - ADVICE r5). */
typedef struct stage_inflight { char *key; uint32_t counter; struct stage_inflight *next; } stage_inflight;
static stage_inflight *g_inflight;                                       /* (g_shared_stage_mu) */
static pthread_mutex_t g_shared_stage_mu = PTHREAD_MUTEX_INITIALIZER;    /* guards g_inflight only: never held across a staging pass */
static pthread_cond_t g_stage_cv = PTHREAD_COND_INITIALIZER;
static long long g_shared_attached, g_shared_published;                  /* (g_shared_mu) */

static int shared_enabled(void) {
    const char *e = getenv("VECTORGPU_SHARE");
    return !(e && *e == '0');
}

/* a reference to the copy (key, counter), or NULL */
static shared_corpus *shared_find_ref(const char *key, uint32_t counter) {
    pthread_mutex_lock(&g_shared_mu);
    shared_corpus *e = g_shared;
    while (e && !(e->counter == counter && !strcmp(e->key, key))) e = e->next;
    if (e) { ++e->refs; ++g_shared_attached; }
    pthread_mutex_unlock(&g_shared_mu);
    return e;
}

static shared_corpus *shared_find_ref(const char *key, uint32_t counter);
/* Either a reference to the published copy (key, counter) - *mine = 0 - or the right to stage it - NULL, *mine = 1 (then the caller MUST
 * call shared_stage_end) - or NULL, *mine = 0 when the bookkeeping ran out of memory (stage privately, publish nothing).  Waits while
 * ANOTHER connection stages exactly this copy. */
static shared_corpus *shared_stage_begin(const char *key, uint32_t counter, int *mine) {
    *mine = 0;
    pthread_mutex_lock(&g_shared_stage_mu);
    for (;;) {
        shared_corpus *e = shared_find_ref(key, counter);
        if (e) { pthread_mutex_unlock(&g_shared_stage_mu); return e; }
        stage_inflight *f = g_inflight;
        while (f && !(f->counter == counter && !strcmp(f->key, key))) f = f->next;
        if (!f) break;
        pthread_cond_wait(&g_stage_cv, &g_shared_stage_mu);             /* the same copy is being staged: wait for that pass, then look again */
    }
    stage_inflight *f = (stage_inflight *)sqlite3_malloc(sizeof(stage_inflight));
    if (f) { f->key = sqlite3_mprintf("%s", key); if (!f->key) { sqlite3_free(f); f = NULL; } }
    if (f) { f->counter = counter; f->next = g_inflight; g_inflight = f; *mine = 1; }
    pthread_mutex_unlock(&g_shared_stage_mu);
    return NULL;
}
/* the staging pass of (key, counter) is over - published or not: whoever waited for it looks again */
static void shared_stage_end(const char *key, uint32_t counter) {
    pthread_mutex_lock(&g_shared_stage_mu);
    stage_inflight **pp = &g_inflight;
    while (*pp && !((*pp)->counter == counter && !strcmp((*pp)->key, key))) pp = &(*pp)->next;
    if (*pp) { stage_inflight *f = *pp; *pp = f->next; sqlite3_free(f->key); sqlite3_free(f); }
    pthread_cond_broadcast(&g_stage_cv);
    pthread_mutex_unlock(&g_shared_stage_mu);
}
/* the counter a shared copy is published under (relabelled under g_shared_mu after vector_quantize's own commit) */
static uint32_t shared_counter_of(shared_corpus *e) {
    pthread_mutex_lock(&g_shared_mu);
    const uint32_t c = e->counter;
    pthread_mutex_unlock(&g_shared_mu);
    return c;
}
/* PRAGMA main.locking_mode = exclusive: the connection keeps its lock between transactions and SQLite does not bump the change counter
 * for each of them - the one mode in which this connection's own committed writes can leave the counter where it was */
static int main_locking_exclusive(sqlite3 *db) {
    sqlite3_stmt *st = NULL;
    int ex = 1;                                                          /* (no answer: assume the worst) */
    if (sqlite3_prepare_v2(db, "PRAGMA main.locking_mode;", -1, &st, NULL) == SQLITE_OK && sqlite3_step(st) == SQLITE_ROW) {
        const char *m = (const char *)sqlite3_column_text(st, 0);
        ex = !(m && strcasecmp(m, "normal") == 0);
    }
    sqlite3_finalize(st);
    return ex;
}

/* a private corpus becomes the shared copy (key, counter); the caller holds the first reference.  NULL: out of memory (it stays private) */
static shared_corpus *shared_publish(const char *key, uint32_t counter, vg_shards *corpus, int64_t table_rows, int64_t max_pk, int have_pk) {
    shared_corpus *e = (shared_corpus *)sqlite3_malloc(sizeof(shared_corpus));
    if (!e) return NULL;
    memset(e, 0, sizeof(*e));
    e->key = sqlite3_mprintf("%s", key);
    if (!e->key) { sqlite3_free(e); return NULL; }
    e->counter = counter; e->corpus = corpus; e->refs = 1;
    e->table_rows = table_rows; e->max_pk = max_pk; e->have_pk = have_pk;
    pthread_mutex_init(&e->mu, NULL);
    pthread_mutex_lock(&g_shared_mu);
    e->next = g_shared;
    g_shared = e;
    ++g_shared_published;
    pthread_mutex_unlock(&g_shared_mu);
    return e;
}

static void shared_unlink_locked(shared_corpus *e) {
    shared_corpus **pp = &g_shared;
    while (*pp && *pp != e) pp = &(*pp)->next;
    if (*pp) *pp = e->next;
}

/* drop a reference; the last one frees the device memory */
static void shared_unref(shared_corpus *e) {
    pthread_mutex_lock(&g_shared_mu);
    const int last = --e->refs == 0;
    if (last) shared_unlink_locked(e);
    pthread_mutex_unlock(&g_shared_mu);
    if (last) {
        G.corpus_destroy(e->corpus);
        pthread_mutex_destroy(&e->mu);
        sqlite3_free(e->key);
        sqlite3_free(e);
    }
}

/* the only holder takes the corpus back (it may be changed again); NULL when others hold it too: such a holder KEEPS its reference (the
 * caller copies the rows - copy-on-write - and drops it then) */
static vg_shards *shared_take_private_or_keep(shared_corpus *e) {
    pthread_mutex_lock(&g_shared_mu);
    const int only = e->refs == 1;
    if (only) shared_unlink_locked(e);
    pthread_mutex_unlock(&g_shared_mu);
    if (!only) return NULL;
    vg_shards *c = e->corpus;
    pthread_mutex_destroy(&e->mu);
    sqlite3_free(e->key);
    sqlite3_free(e);
    return c;
}

/* Can this connection share copies of `table` right now, and under which counter?  Takes a SHARED lock for the read of page 1 (through
 * SQLite's own file handle: a second descriptor on the database file, once closed, would drop the process' POSIX locks on it). */
static int shared_probe(sqlite3 *db, const char *table, uint32_t *counter, char *file_id, size_t file_id_size) {
    if (!shared_enabled() || !sqlite3_get_autocommit(db)) return 0;
    const char *fn = sqlite3_db_filename(db, "main");
    if (!fn || !*fn) return 0;                                           /* in-memory / temporary database */
    sqlite3_stmt *st = NULL;
    int ok = 0;
    if (sqlite3_prepare_v2(db, "PRAGMA main.journal_mode;", -1, &st, NULL) == SQLITE_OK && sqlite3_step(st) == SQLITE_ROW) {
        const char *jm = (const char *)sqlite3_column_text(st, 0);
        ok = jm && strcasecmp(jm, "wal") != 0;
    }
    sqlite3_finalize(st);
    st = NULL;
    if (!ok) return 0;
    /* the table is main's own and no TEMP table hides it */
    ok = 0;
    if (sqlite3_prepare_v2(db, "SELECT (SELECT count(*) FROM main.sqlite_master WHERE type='table' AND name=?1 COLLATE NOCASE),"
                               " (SELECT count(*) FROM temp.sqlite_master WHERE name=?1 COLLATE NOCASE);", -1, &st, NULL) != SQLITE_OK) { sqlite3_finalize(st); return 0; }
    sqlite3_bind_text(st, 1, table, -1, SQLITE_STATIC);
    if (sqlite3_step(st) == SQLITE_ROW)                                  /* (the statement stays active: the SHARED lock is held until it is finalized) */
        ok = sqlite3_column_int(st, 0) == 1 && sqlite3_column_int(st, 1) == 0;
    if (ok) {
        sqlite3_file *f = NULL;
        int moved = 0;
        unsigned char hdr[100];
        struct stat sb;
        ok = sqlite3_file_control(db, "main", SQLITE_FCNTL_FILE_POINTER, &f) == SQLITE_OK && f && f->pMethods &&
             sqlite3_file_control(db, "main", SQLITE_FCNTL_HAS_MOVED, &moved) == SQLITE_OK && !moved &&
             f->pMethods->xRead(f, hdr, (int)sizeof(hdr), 0) == SQLITE_OK && stat(fn, &sb) == 0;
        if (ok) {
            *counter = ((uint32_t)hdr[24] << 24) | ((uint32_t)hdr[25] << 16) | ((uint32_t)hdr[26] << 8) | (uint32_t)hdr[27];
            snprintf(file_id, file_id_size, "%s#%llu:%llu", fn, (unsigned long long)sb.st_dev, (unsigned long long)sb.st_ino);
        }
    }
    sqlite3_finalize(st);
    return ok;
}

/* vext_sqlite.h - the part of SQLite's public C interface (https://sqlite.org/c3ref/intro.html) that vector_ext.c uses, so that the
 * extension builds without SQLite's development headers.
 *
 * Like any loadable extension, vector.so calls SQLite only through the routines table its host hands to the entry point
 * (sqlite3_api_routines): it works in every host, whether SQLite is a shared library or compiled in, and links no SQLite of its own.
 * Only what the extension uses is declared here; the values, the layouts and the table's order are SQLite's stable ABI (the
 * virtual-table structures as of iVersion 3, sqlite3_index_info as of 3.10, the routines table up to txn_state, 3.34).
 */
#ifndef VEXT_SQLITE_H
#define VEXT_SQLITE_H

#include <stdarg.h>

typedef long long int sqlite3_int64;
typedef unsigned long long int sqlite3_uint64;

typedef struct sqlite3 sqlite3;
typedef struct sqlite3_stmt sqlite3_stmt;
typedef struct sqlite3_value sqlite3_value;
typedef struct sqlite3_context sqlite3_context;
typedef struct sqlite3_mutex sqlite3_mutex;
typedef struct sqlite3_api_routines sqlite3_api_routines;
typedef void (*sqlite3_destructor_type)(void *);

/* result codes */
#define SQLITE_OK 0
#define SQLITE_ERROR 1
#define SQLITE_NOMEM 7
#define SQLITE_ROW 100
#define SQLITE_DONE 101

/* fundamental datatypes */
#define SQLITE_INTEGER 1
#define SQLITE_FLOAT 2
#define SQLITE_TEXT 3
#define SQLITE_BLOB 4
#define SQLITE_NULL 5

#define SQLITE_UTF8 1
#define SQLITE_STATIC ((sqlite3_destructor_type)0)
#define SQLITE_TRANSIENT ((sqlite3_destructor_type)-1)

#define SQLITE_OPEN_READONLY 0x00000001
#define SQLITE_OPEN_NOMUTEX 0x00008000
#define SQLITE_MUTEX_FAST 0
#define SQLITE_INDEX_CONSTRAINT_EQ 2
#define SQLITE_FCNTL_FILE_POINTER 7
#define SQLITE_FCNTL_HAS_MOVED 20
#define SQLITE_TXN_NONE 0

/* an open file of a VFS: only the leading members are declared - the extension reads them through a pointer SQLite hands it and
 * never creates one */
typedef struct sqlite3_file sqlite3_file;
typedef struct sqlite3_io_methods {
    int iVersion;
    int (*xClose)(sqlite3_file *);
    int (*xRead)(sqlite3_file *, void *, int iAmt, sqlite3_int64 iOfst);
} sqlite3_io_methods;
struct sqlite3_file {
    const sqlite3_io_methods *pMethods;
};

/* virtual tables */
typedef struct sqlite3_vtab sqlite3_vtab;
typedef struct sqlite3_vtab_cursor sqlite3_vtab_cursor;
typedef struct sqlite3_index_info sqlite3_index_info;
typedef struct sqlite3_module sqlite3_module;

struct sqlite3_module {
    int iVersion;
    int (*xCreate)(sqlite3 *, void *pAux, int argc, const char *const *argv, sqlite3_vtab **ppVTab, char **pzErr);
    int (*xConnect)(sqlite3 *, void *pAux, int argc, const char *const *argv, sqlite3_vtab **ppVTab, char **pzErr);
    int (*xBestIndex)(sqlite3_vtab *, sqlite3_index_info *);
    int (*xDisconnect)(sqlite3_vtab *);
    int (*xDestroy)(sqlite3_vtab *);
    int (*xOpen)(sqlite3_vtab *, sqlite3_vtab_cursor **);
    int (*xClose)(sqlite3_vtab_cursor *);
    int (*xFilter)(sqlite3_vtab_cursor *, int idxNum, const char *idxStr, int argc, sqlite3_value **argv);
    int (*xNext)(sqlite3_vtab_cursor *);
    int (*xEof)(sqlite3_vtab_cursor *);
    int (*xColumn)(sqlite3_vtab_cursor *, sqlite3_context *, int);
    int (*xRowid)(sqlite3_vtab_cursor *, sqlite3_int64 *);
    int (*xUpdate)(sqlite3_vtab *, int, sqlite3_value **, sqlite3_int64 *);
    int (*xBegin)(sqlite3_vtab *);
    int (*xSync)(sqlite3_vtab *);
    int (*xCommit)(sqlite3_vtab *);
    int (*xRollback)(sqlite3_vtab *);
    int (*xFindFunction)(sqlite3_vtab *, int nArg, const char *zName, void (**pxFunc)(sqlite3_context *, int, sqlite3_value **), void **ppArg);
    int (*xRename)(sqlite3_vtab *, const char *zNew);
    int (*xSavepoint)(sqlite3_vtab *, int);
    int (*xRelease)(sqlite3_vtab *, int);
    int (*xRollbackTo)(sqlite3_vtab *, int);
    int (*xShadowName)(const char *);
};

struct sqlite3_index_info {
    int nConstraint;
    struct sqlite3_index_constraint {
        int iColumn;
        unsigned char op;
        unsigned char usable;
        int iTermOffset;
    } *aConstraint;
    int nOrderBy;
    struct sqlite3_index_orderby {
        int iColumn;
        unsigned char desc;
    } *aOrderBy;
    struct sqlite3_index_constraint_usage {
        int argvIndex;
        unsigned char omit;
    } *aConstraintUsage;
    int idxNum;
    char *idxStr;
    int needToFreeIdxStr;
    int orderByConsumed;
    double estimatedCost;
    sqlite3_int64 estimatedRows;
    int idxFlags;
    sqlite3_uint64 colUsed;
};

struct sqlite3_vtab {
    const sqlite3_module *pModule;
    int nRef;
    char *zErrMsg;
};

struct sqlite3_vtab_cursor {
    sqlite3_vtab *pVtab;
};

/* SQLite's prototypes: they give the table's entries their types (below); nothing calls these symbols directly */

/* memory and strings */
void *sqlite3_malloc(int);
void *sqlite3_malloc64(sqlite3_uint64);
void *sqlite3_realloc64(void *, sqlite3_uint64);
void sqlite3_free(void *);
char *sqlite3_mprintf(const char *, ...);
char *sqlite3_vmprintf(const char *, va_list);
char *sqlite3_snprintf(int, char *, const char *, ...);
int sqlite3_stricmp(const char *, const char *);

/* the library and its connections */
int sqlite3_libversion_number(void);
int sqlite3_threadsafe(void);
sqlite3_mutex *sqlite3_mutex_alloc(int);
void sqlite3_mutex_free(sqlite3_mutex *);
int sqlite3_open_v2(const char *filename, sqlite3 **ppDb, int flags, const char *zVfs);
int sqlite3_close(sqlite3 *);
int sqlite3_busy_timeout(sqlite3 *, int ms);
int sqlite3_exec(sqlite3 *, const char *sql, int (*callback)(void *, int, char **, char **), void *, char **errmsg);
const char *sqlite3_errmsg(sqlite3 *);
int sqlite3_get_autocommit(sqlite3 *);
int sqlite3_total_changes(sqlite3 *);
int sqlite3_txn_state(sqlite3 *, const char *zSchema);
const char *sqlite3_db_filename(sqlite3 *, const char *zDbName);
int sqlite3_file_control(sqlite3 *, const char *zDbName, int op, void *);
void *sqlite3_update_hook(sqlite3 *, void (*)(void *, int, const char *, const char *, sqlite3_int64), void *);

/* statements */
int sqlite3_prepare_v2(sqlite3 *, const char *zSql, int nByte, sqlite3_stmt **ppStmt, const char **pzTail);
int sqlite3_step(sqlite3_stmt *);
int sqlite3_reset(sqlite3_stmt *);
int sqlite3_finalize(sqlite3_stmt *);
int sqlite3_stmt_readonly(sqlite3_stmt *);
int sqlite3_bind_blob(sqlite3_stmt *, int, const void *, int n, void (*)(void *));
int sqlite3_bind_double(sqlite3_stmt *, int, double);
int sqlite3_bind_int(sqlite3_stmt *, int, int);
int sqlite3_bind_int64(sqlite3_stmt *, int, sqlite3_int64);
int sqlite3_bind_text(sqlite3_stmt *, int, const char *, int, void (*)(void *));
const void *sqlite3_column_blob(sqlite3_stmt *, int iCol);
int sqlite3_column_bytes(sqlite3_stmt *, int iCol);
int sqlite3_column_count(sqlite3_stmt *);
double sqlite3_column_double(sqlite3_stmt *, int iCol);
int sqlite3_column_int(sqlite3_stmt *, int iCol);
sqlite3_int64 sqlite3_column_int64(sqlite3_stmt *, int iCol);
const unsigned char *sqlite3_column_text(sqlite3_stmt *, int iCol);
int sqlite3_column_type(sqlite3_stmt *, int iCol);

/* SQL functions: arguments and results */
const void *sqlite3_value_blob(sqlite3_value *);
int sqlite3_value_bytes(sqlite3_value *);
double sqlite3_value_double(sqlite3_value *);
int sqlite3_value_int(sqlite3_value *);
sqlite3_int64 sqlite3_value_int64(sqlite3_value *);
const unsigned char *sqlite3_value_text(sqlite3_value *);
int sqlite3_value_type(sqlite3_value *);
void *sqlite3_user_data(sqlite3_context *);
sqlite3 *sqlite3_context_db_handle(sqlite3_context *);
void sqlite3_result_blob(sqlite3_context *, const void *, int, void (*)(void *));
void sqlite3_result_double(sqlite3_context *, double);
void sqlite3_result_error(sqlite3_context *, const char *, int);
void sqlite3_result_error_code(sqlite3_context *, int);
void sqlite3_result_error_nomem(sqlite3_context *);
void sqlite3_result_int(sqlite3_context *, int);
void sqlite3_result_int64(sqlite3_context *, sqlite3_int64);
void sqlite3_result_text(sqlite3_context *, const char *, int, void (*)(void *));
void sqlite3_result_value(sqlite3_context *, sqlite3_value *);

/* registration */
int sqlite3_create_function(sqlite3 *, const char *zFunctionName, int nArg, int eTextRep, void *pApp,
                            void (*xFunc)(sqlite3_context *, int, sqlite3_value **),
                            void (*xStep)(sqlite3_context *, int, sqlite3_value **),
                            void (*xFinal)(sqlite3_context *));
int sqlite3_create_function_v2(sqlite3 *, const char *zFunctionName, int nArg, int eTextRep, void *pApp,
                               void (*xFunc)(sqlite3_context *, int, sqlite3_value **),
                               void (*xStep)(sqlite3_context *, int, sqlite3_value **),
                               void (*xFinal)(sqlite3_context *),
                               void (*xDestroy)(void *));
int sqlite3_create_module(sqlite3 *, const char *zName, const sqlite3_module *, void *pClientData);
int sqlite3_declare_vtab(sqlite3 *, const char *zSQL);

/* The host's routines table: one function pointer per entry, in SQLite's order.  Entries this extension calls are named after their
 * function; the others are left as unused_<first entry>[<count>].  Entries past txn_state are not declared. */
struct sqlite3_api_routines {
    void *unused_0[2];
    __typeof__(sqlite3_bind_blob) *sqlite3_bind_blob;
    __typeof__(sqlite3_bind_double) *sqlite3_bind_double;
    __typeof__(sqlite3_bind_int) *sqlite3_bind_int;
    __typeof__(sqlite3_bind_int64) *sqlite3_bind_int64;
    void *unused_6[4];
    __typeof__(sqlite3_bind_text) *sqlite3_bind_text;
    void *unused_11[3];
    __typeof__(sqlite3_busy_timeout) *sqlite3_busy_timeout;
    void *unused_15[1];
    __typeof__(sqlite3_close) *sqlite3_close;
    void *unused_17[2];
    __typeof__(sqlite3_column_blob) *sqlite3_column_blob;
    __typeof__(sqlite3_column_bytes) *sqlite3_column_bytes;
    void *unused_21[1];
    __typeof__(sqlite3_column_count) *sqlite3_column_count;
    void *unused_23[4];
    __typeof__(sqlite3_column_double) *sqlite3_column_double;
    __typeof__(sqlite3_column_int) *sqlite3_column_int;
    __typeof__(sqlite3_column_int64) *sqlite3_column_int64;
    void *unused_30[6];
    __typeof__(sqlite3_column_text) *sqlite3_column_text;
    void *unused_37[1];
    __typeof__(sqlite3_column_type) *sqlite3_column_type;
    void *unused_39[6];
    __typeof__(sqlite3_create_function) *sqlite3_create_function;
    void *unused_46[1];
    __typeof__(sqlite3_create_module) *sqlite3_create_module;
    void *unused_48[2];
    __typeof__(sqlite3_declare_vtab) *sqlite3_declare_vtab;
    void *unused_51[2];
    __typeof__(sqlite3_errmsg) *sqlite3_errmsg;
    void *unused_54[1];
    __typeof__(sqlite3_exec) *sqlite3_exec;
    void *unused_56[1];
    __typeof__(sqlite3_finalize) *sqlite3_finalize;
    __typeof__(sqlite3_free) *sqlite3_free;
    void *unused_59[1];
    __typeof__(sqlite3_get_autocommit) *sqlite3_get_autocommit;
    void *unused_61[6];
    __typeof__(sqlite3_libversion_number) *sqlite3_libversion_number;
    __typeof__(sqlite3_malloc) *sqlite3_malloc;
    __typeof__(sqlite3_mprintf) *sqlite3_mprintf;
    void *unused_70[7];
    __typeof__(sqlite3_reset) *sqlite3_reset;
    __typeof__(sqlite3_result_blob) *sqlite3_result_blob;
    __typeof__(sqlite3_result_double) *sqlite3_result_double;
    __typeof__(sqlite3_result_error) *sqlite3_result_error;
    void *unused_81[1];
    __typeof__(sqlite3_result_int) *sqlite3_result_int;
    __typeof__(sqlite3_result_int64) *sqlite3_result_int64;
    void *unused_84[1];
    __typeof__(sqlite3_result_text) *sqlite3_result_text;
    void *unused_86[3];
    __typeof__(sqlite3_result_value) *sqlite3_result_value;
    void *unused_90[3];
    __typeof__(sqlite3_snprintf) *sqlite3_snprintf;
    __typeof__(sqlite3_step) *sqlite3_step;
    void *unused_95[2];
    __typeof__(sqlite3_total_changes) *sqlite3_total_changes;
    void *unused_98[2];
    __typeof__(sqlite3_update_hook) *sqlite3_update_hook;
    __typeof__(sqlite3_user_data) *sqlite3_user_data;
    __typeof__(sqlite3_value_blob) *sqlite3_value_blob;
    __typeof__(sqlite3_value_bytes) *sqlite3_value_bytes;
    void *unused_104[1];
    __typeof__(sqlite3_value_double) *sqlite3_value_double;
    __typeof__(sqlite3_value_int) *sqlite3_value_int;
    __typeof__(sqlite3_value_int64) *sqlite3_value_int64;
    void *unused_108[1];
    __typeof__(sqlite3_value_text) *sqlite3_value_text;
    void *unused_110[3];
    __typeof__(sqlite3_value_type) *sqlite3_value_type;
    __typeof__(sqlite3_vmprintf) *sqlite3_vmprintf;
    void *unused_115[1];
    __typeof__(sqlite3_prepare_v2) *sqlite3_prepare_v2;
    void *unused_117[10];
    __typeof__(sqlite3_file_control) *sqlite3_file_control;
    void *unused_128[2];
    __typeof__(sqlite3_mutex_alloc) *sqlite3_mutex_alloc;
    void *unused_131[1];
    __typeof__(sqlite3_mutex_free) *sqlite3_mutex_free;
    void *unused_133[2];
    __typeof__(sqlite3_open_v2) *sqlite3_open_v2;
    void *unused_136[1];
    __typeof__(sqlite3_result_error_nomem) *sqlite3_result_error_nomem;
    void *unused_138[6];
    __typeof__(sqlite3_threadsafe) *sqlite3_threadsafe;
    void *unused_145[1];
    __typeof__(sqlite3_result_error_code) *sqlite3_result_error_code;
    void *unused_147[2];
    __typeof__(sqlite3_context_db_handle) *sqlite3_context_db_handle;
    void *unused_150[12];
    __typeof__(sqlite3_create_function_v2) *sqlite3_create_function_v2;
    void *unused_163[17];
    __typeof__(sqlite3_db_filename) *sqlite3_db_filename;
    void *unused_181[4];
    __typeof__(sqlite3_stmt_readonly) *sqlite3_stmt_readonly;
    __typeof__(sqlite3_stricmp) *sqlite3_stricmp;
    void *unused_187[10];
    __typeof__(sqlite3_malloc64) *sqlite3_malloc64;
    void *unused_198[1];
    __typeof__(sqlite3_realloc64) *sqlite3_realloc64;
    void *unused_200[52];
    __typeof__(sqlite3_txn_state) *sqlite3_txn_state;
};

/* every call below goes through the host's table */
#define sqlite3_bind_blob            sqlite3_api->sqlite3_bind_blob
#define sqlite3_bind_double          sqlite3_api->sqlite3_bind_double
#define sqlite3_bind_int             sqlite3_api->sqlite3_bind_int
#define sqlite3_bind_int64           sqlite3_api->sqlite3_bind_int64
#define sqlite3_bind_text            sqlite3_api->sqlite3_bind_text
#define sqlite3_busy_timeout         sqlite3_api->sqlite3_busy_timeout
#define sqlite3_close                sqlite3_api->sqlite3_close
#define sqlite3_column_blob          sqlite3_api->sqlite3_column_blob
#define sqlite3_column_bytes         sqlite3_api->sqlite3_column_bytes
#define sqlite3_column_count         sqlite3_api->sqlite3_column_count
#define sqlite3_column_double        sqlite3_api->sqlite3_column_double
#define sqlite3_column_int           sqlite3_api->sqlite3_column_int
#define sqlite3_column_int64         sqlite3_api->sqlite3_column_int64
#define sqlite3_column_text          sqlite3_api->sqlite3_column_text
#define sqlite3_column_type          sqlite3_api->sqlite3_column_type
#define sqlite3_context_db_handle    sqlite3_api->sqlite3_context_db_handle
#define sqlite3_create_function      sqlite3_api->sqlite3_create_function
#define sqlite3_create_function_v2   sqlite3_api->sqlite3_create_function_v2
#define sqlite3_create_module        sqlite3_api->sqlite3_create_module
#define sqlite3_db_filename          sqlite3_api->sqlite3_db_filename
#define sqlite3_declare_vtab         sqlite3_api->sqlite3_declare_vtab
#define sqlite3_errmsg               sqlite3_api->sqlite3_errmsg
#define sqlite3_exec                 sqlite3_api->sqlite3_exec
#define sqlite3_file_control         sqlite3_api->sqlite3_file_control
#define sqlite3_finalize             sqlite3_api->sqlite3_finalize
#define sqlite3_free                 sqlite3_api->sqlite3_free
#define sqlite3_get_autocommit       sqlite3_api->sqlite3_get_autocommit
#define sqlite3_libversion_number    sqlite3_api->sqlite3_libversion_number
#define sqlite3_malloc               sqlite3_api->sqlite3_malloc
#define sqlite3_malloc64             sqlite3_api->sqlite3_malloc64
#define sqlite3_mprintf              sqlite3_api->sqlite3_mprintf
#define sqlite3_mutex_alloc          sqlite3_api->sqlite3_mutex_alloc
#define sqlite3_mutex_free           sqlite3_api->sqlite3_mutex_free
#define sqlite3_open_v2              sqlite3_api->sqlite3_open_v2
#define sqlite3_prepare_v2           sqlite3_api->sqlite3_prepare_v2
#define sqlite3_realloc64            sqlite3_api->sqlite3_realloc64
#define sqlite3_reset                sqlite3_api->sqlite3_reset
#define sqlite3_result_blob          sqlite3_api->sqlite3_result_blob
#define sqlite3_result_double        sqlite3_api->sqlite3_result_double
#define sqlite3_result_error         sqlite3_api->sqlite3_result_error
#define sqlite3_result_error_code    sqlite3_api->sqlite3_result_error_code
#define sqlite3_result_error_nomem   sqlite3_api->sqlite3_result_error_nomem
#define sqlite3_result_int           sqlite3_api->sqlite3_result_int
#define sqlite3_result_int64         sqlite3_api->sqlite3_result_int64
#define sqlite3_result_text          sqlite3_api->sqlite3_result_text
#define sqlite3_result_value         sqlite3_api->sqlite3_result_value
#define sqlite3_snprintf             sqlite3_api->sqlite3_snprintf
#define sqlite3_step                 sqlite3_api->sqlite3_step
#define sqlite3_stmt_readonly        sqlite3_api->sqlite3_stmt_readonly
#define sqlite3_stricmp              sqlite3_api->sqlite3_stricmp
#define sqlite3_threadsafe           sqlite3_api->sqlite3_threadsafe
#define sqlite3_total_changes        sqlite3_api->sqlite3_total_changes
#define sqlite3_txn_state            sqlite3_api->sqlite3_txn_state
#define sqlite3_update_hook          sqlite3_api->sqlite3_update_hook
#define sqlite3_user_data            sqlite3_api->sqlite3_user_data
#define sqlite3_value_blob           sqlite3_api->sqlite3_value_blob
#define sqlite3_value_bytes          sqlite3_api->sqlite3_value_bytes
#define sqlite3_value_double         sqlite3_api->sqlite3_value_double
#define sqlite3_value_int            sqlite3_api->sqlite3_value_int
#define sqlite3_value_int64          sqlite3_api->sqlite3_value_int64
#define sqlite3_value_text           sqlite3_api->sqlite3_value_text
#define sqlite3_value_type           sqlite3_api->sqlite3_value_type
#define sqlite3_vmprintf             sqlite3_api->sqlite3_vmprintf

/* the one global an extension keeps: the table, stored by the entry point */
#define SQLITE_EXTENSION_INIT1 const sqlite3_api_routines *sqlite3_api = 0;
extern const sqlite3_api_routines *sqlite3_api;

#endif

/*
 * resql_hip.h — C ABI of the MI355X-native execution engine for ReSQL operator pipelines.
 *
 * This library takes the place of ReSQL's JIT context: where the reference's
 * `executeSelectPlan` (reference src/execute.h:213-247) does
 *
 *     JitContextFlounder ctx ( config.jit );            // src/JitContextFlounder.h:228
 *     root->produceFlounder ( ctx, {} );                // operators emit Flounder IR
 *     ctx.compile();                                    // src/JitContextFlounder.h:410-456
 *     ctx.execute();                                    // src/JitContextFlounder.h:459-487
 *     rel = root->retrieveResult();                     // operators/materialize.h:48, orderby.h:87
 *
 * a host links this library and does
 *
 *     rsq_ctx_create      -> one engine context per GPU (replaces the JitContextFlounder ctor)
 *     rsq_table_create*   -> columns resident in HBM (replaces Relation / DataBlock row store,
 *                            src/dbdata.h:23-461, as the scan source; scan.h:85-166)
 *     rsq_query_compile   -> describe + compile: type derivation, pipeline extraction, HIP kernel
 *                            specialisation (replaces produceFlounder + ctx.compile())
 *     rsq_query_execute   -> launch the pipelines' kernels, synchronise (replaces ctx.execute())
 *     rsq_query_result    -> packed result tuples in ReSQL's own layout (replaces retrieveResult())
 *
 * Everything is plain C: opaque handles, plain pointers and sizes, int status codes.  No
 * exceptions cross the boundary and the library never calls exit() (the reference's
 * query_error() does, src/qlib/error.h:29-68): errors come back as a status code plus
 * rsq_last_error().
 *
 * The plan / table / result structs are in resql_plan.h.
 */
#ifndef RESQL_HIP_H
#define RESQL_HIP_H

#include "resql_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsq_ctx   rsq_ctx;
typedef struct rsq_table rsq_table;
typedef struct rsq_query rsq_query;

enum rsq_status {
    RSQ_OK = 0,
    RSQ_ERR_INVALID = 1,        /* malformed plan / arguments */
    RSQ_ERR_TYPE = 2,           /* what the reference reports as ResqlError during type derivation / codegen */
    RSQ_ERR_UNSUPPORTED = 3,    /* valid ReSQL plan, pipeline shape not implemented by this engine */
    RSQ_ERR_DEVICE = 4,         /* HIP runtime / compiler failure, no usable GPU */
    RSQ_ERR_RUNTIME = 5,        /* query-time error (division by zero, hash table full, ...) */
    RSQ_ERR_NOMEM = 6
};

/* Mirrors JitConfig (reference src/JitContextFlounder.h:86-109) field for field — behind `struct_size` — plus the device and the
 * engine's own settings.  struct_size = sizeof(rsq_config) of the header the HOST was compiled against: the library reads that many
 * bytes and takes every later field as 0, so the struct can grow without a host built against an older header handing over
 * garbage (0 is refused: an uninitialised struct). */
typedef struct rsq_config {
    uint32_t struct_size;        /* sizeof(rsq_config) */
    int32_t print_assembly;      /* JitConfig::printAssembly  -> dump generated HIP source */
    int32_t print_flounder;      /* JitConfig::printFlounder  -> dump the pipeline description */
    int32_t print_performance;   /* JitConfig::printPerformance */
    int32_t num_threads;         /* JitConfig::numThreads: host threads of the CPU path; unused by the GPU engine */
    int32_t emit_machine_code;   /* JitConfig::emitMachineCode: ignored (always in-process code objects) */
    int32_t optimize;            /* JitConfig::optimizeFlounder: ignored */
    int32_t device;              /* HIP device ordinal this context drives (one context per GPU / process) */
    const char* kernel_cache_dir;/* directory with pre-built code objects (NULL: <library dir>/../_kcache) */
    int32_t emission_order;      /* rsq_emission_order: order of an aggregation's rows when the plan does not sort them */
    uint32_t compat_flags;       /* rsq_compat bits: where "as the reference's source says" and "as its JIT executes" differ */
    uint32_t engine_flags;       /* rsq_engine_flags bits (0: the defaults) */
    uint32_t reserved0;
    int64_t  arena_reserve_bytes;/* device memory the context takes from the driver when it is created, for the tables and buffers of its
                                  * queries (0: 2 GiB, and 40 MiB of pinned host memory; < 0: nothing up front - slabs are taken when first needed) */
    int64_t  arena_keep_bytes;   /* free arena memory the context keeps between queries before slabs go back to the driver (0: 1/8 of the
                                  * device's memory) */
    int64_t  nested_loops_max_pairs;/* RSQ_ENGINE_NESTED_LOOPS: most (outer rows x inner rows) one nested-loops join may pair; an execution
                                  * beyond it is RSQ_ERR_UNSUPPORTED before any pair is formed (0: 2^36; < 0: RSQ_ERR_INVALID) */
    int32_t nested_loops_inner_slices;   /* 0: chosen per execution; 1: never split; 2..4096: that many (at most the grid cap); else RSQ_ERR_INVALID */
    int32_t tbl_ingest;          /* where BULK INSERT parses its '.tbl' text: 0 host threads, 1 the device (rsq_table_load_tbl_ex below);
                                  * else RSQ_ERR_INVALID */
} rsq_config;

/* A ReSQL host compiles a statement, executes it ONCE and deletes the plan (reference src/execute.h:213-247).  Two things make that one
 * execution cost what a repeated one costs, both owned by the context and both on by default:
 *   - memory arenas: join / aggregation tables, group rows and pinned read-back buffers of a query are ranges of slabs the context took
 *     from the driver once (hipMalloc / hipFree / hipHostMalloc cost more than a whole TPC-H Q3 at SF10).  RSQ_ENGINE_DRIVER_ALLOC takes
 *     every buffer from the driver instead;
 *   - the plan memo: what an execution learns about a plan over a table version - build cardinalities, whether build keys are unique
 *     (rank dictionary or hash form), group counts, region layouts of a staged aggregation, result sizes, which kernel form ran - is
 *     kept by (kernel texts, table ids + versions) and a later query of the same shape starts with it; everything in it is re-checked by
 *     the execution (a stale entry costs a repeated execution, never a wrong answer).  RSQ_ENGINE_NO_PLAN_MEMO starts every query cold.
 * RSQ_ENGINE_NESTED_LOOPS (off by default) lets the context plan and execute nested-loops joins (planner.h:458-469: FROM lists whose
 * tables are not all linked by equalities; RSQ_OP_NESTEDLOOPSJOIN in a plan description).  Such a join costs outer x inner pairs, so
 * a host enables it explicitly and bounds it with rsq_config.nested_loops_max_pairs.  Without the flag those plans are refused
 * (RSQ_ERR_UNSUPPORTED) as before.
 * The reference folds FROM pieces in creation order, so `from big, small` pairs FEW outer rows with MANY inner rows, and the outer rows
 * alone do not fill a GPU.  A join whose pairs end in an aggregation therefore splits its inner rows into S slices at launch: S workgroups
 * per group of outer rows, each pairing those rows with one slice (rsq_config.nested_loops_inner_slices; the policy is
 * rsq_nested_loops_slices below, the S of an execution rsq_query_nested_loops_slices).  Sums, counts, minima, maxima and a group's first
 * pair merge in any order, so the result is the same bytes for every S.  A join whose pairs are materialised, or fill a hash join's
 * build side, keeps S = 1: their output positions follow the scan order.
 * RSQ_ENGINE_DERIVED_MULTI (off by default) lets a multi-GPU handle (rsq_multi_config.base) run plans with derived aggregations; see
 * rsq_multi_* below.  It is a setting of multi-GPU handles only: rsq_ctx_create refuses it (one context runs such plans without it).
 * RSQ_ENGINE_DICT_MULTI (off by default; a setting of multi-GPU handles only, like the one above) gives the shards of a table ONE
 * dictionary per dictionary-coded string column (the union of the shards' dictionaries, rsq_table_unify_shard_dictionaries) when a
 * statement is compiled, so that a GROUP BY over such a column is a dense table keyed by the code on every shard and merges as dense
 * partial tables.  Without it such a statement keeps the hash form across shards.  It has an effect only where the dictionary images
 * are on (RSQ_DICT_SCANS). */
enum rsq_engine_flags { RSQ_ENGINE_DRIVER_ALLOC = 1u, RSQ_ENGINE_NO_PLAN_MEMO = 2u, RSQ_ENGINE_NESTED_LOOPS = 4u, RSQ_ENGINE_DERIVED_MULTI = 8u,
                        RSQ_ENGINE_DICT_MULTI = 16u };

/* Semantics switches.  The default (0) computes what the reference's SOURCE specifies; a bit selects what its asmjit back end
 * actually executes where the two differ, for a drop-in host that must return the JIT's own answers:
 *   RSQ_COMPAT_JIT_INT16_CAST — TYPECAST INT -> BIGINT is a 32 -> 64-bit sign extension in ExpressionsJitFlounder.h:818-824 (`movsx`);
 *     the asmjit translation encodes the 16-bit form, so the JIT extends the LOW 16 BITS (`l_orderkey < 3` also keeps key 65537).
 *     With the bit set device code, interpreter and host tail do the same.
 * Not selectable: ht_get's missing wrap-around (src/qlib/hash.h:427-477) reads one entry past the table's allocation, so what the
 * reference returns for a probe chain that crosses the table's end depends on heap contents; the engine always walks the chain
 * (tests/test_reference_defect.py pins the difference on the live reference). */
enum rsq_compat { RSQ_COMPAT_JIT_INT16_CAST = 1u };

/* Without ORDER BY the reference emits an aggregation's groups in the slot order of its hash table (operators/aggregation.h:
 * 298-343), which depends on the order the groups first occur in the input, its hash function, prime table sizes and growth rule.
 * RSQ_EMIT_REFERENCE (0, the default) reproduces that order exactly — the result relation is byte-identical to ReSQL's — at the
 * price of replaying that table on the host (a few ms per million groups).  RSQ_EMIT_ANY returns the same rows in whatever
 * order the device tables hold them (the reference's own tests compare such results as multisets, test/test_common.h:152-190);
 * ORDER BY still sorts them with the reference's quicksort, but rows that tie on all sort keys may then come in another order. */
enum rsq_emission_order { RSQ_EMIT_REFERENCE = 0, RSQ_EMIT_ANY = 1 };

/* Mirrors JitExecutionReport (reference src/JitContextFlounder.h:114-129), times in ms, plus the
 * GPU-side figures SURVEY.md §8(b) asks for. */
typedef struct rsq_report {
    double   compilation_time_ms;    /* describe + kernel specialisation (JIT or cache hit) */
    double   execution_time_ms;      /* host wall time of rsq_query_execute, launches to final sync */
    double   kernel_time_ms;         /* sum of device kernel durations (HIP events on the engine's stream) */
    double   finalize_time_ms;       /* host-side AVG / projection / order-by / limit over the group rows */
    uint64_t num_kernels;            /* launches issued by the last execute (cf. numMachineInstructions) */
    uint64_t bytes_read;             /* ALGORITHMIC bytes: column bytes the pipelines must read once */
    double   hbm_gbps;               /* bytes_read / kernel_time */
    int32_t  jit_cache_hits;         /* pipelines served from the code-object cache */
    int32_t  jit_compiles;           /* pipelines compiled with hiprtc in this call */
} rsq_report;

/* ---- context ----------------------------------------------------------------------------- */
int  rsq_ctx_create(const rsq_config* cfg, rsq_ctx** out);
void rsq_ctx_destroy(rsq_ctx* ctx);
/* Message of the last failing call on this context (or of rsq_ctx_create when ctx == NULL). */
const char* rsq_last_error(const rsq_ctx* ctx);
/* What the context holds (its arenas, see rsq_engine_flags) and how often it went to the driver: a host that runs statement after
 * statement sees driver calls stop growing once the slabs cover its working set.  struct_size = sizeof(rsq_memory_stats), as in rsq_config. */
typedef struct rsq_memory_stats {
    uint32_t struct_size;
    uint32_t reserved0;
    uint64_t device_slab_bytes;      /* device memory held by the arena */
    uint64_t device_used_bytes;      /* ... of it handed out to live queries */
    uint64_t device_slab_allocs;     /* hipMalloc calls made for slabs since the context was created */
    uint64_t pinned_slab_bytes;      /* pinned host memory held (coherent + non-coherent arenas) */
    uint64_t pinned_used_bytes;
    uint64_t pinned_slab_allocs;     /* hipHostMalloc calls made for slabs */
    uint64_t raw_driver_calls;       /* hipMalloc / hipFree calls outside the arenas (table columns; every buffer with RSQ_ENGINE_DRIVER_ALLOC) */
    uint64_t arena_requests;         /* buffers handed out by the arenas */
    double   driver_ms;              /* host time spent inside those driver calls */
    uint64_t plan_memo_entries;      /* plans the context remembers */
    uint64_t plan_memo_hits;         /* queries that were compiled with a remembered entry */
    uint64_t key_index_entries;      /* key bitmaps of engine-owned key columns kept for every query over the same table version (joins whose build side is that table as it stands) */
    uint64_t key_index_bytes;        /* ... device memory they hold (part of device_used_bytes; freed with the table or when it changes) */
    uint64_t column_image_bytes;     /* device memory of the tables' narrow and dictionary images (straight from the driver, like the columns) */
} rsq_memory_stats;
int  rsq_ctx_memory_stats(const rsq_ctx* ctx, rsq_memory_stats* out);

/* ---- tables ------------------------------------------------------------------------------ */
/* Copy host columns to the device (H2D is outside every timed region). Column statistics the
 * planner uses (row count as Relation::tupleNum(), min/max, byte-value sets) are gathered here. */
int  rsq_table_create(rsq_ctx* ctx, const rsq_table_desc* desc, rsq_table** out);
/* Adopt columns that already live in this GPU's memory (e.g. torch tensors): `data` pointers are
 * device pointers, not copied, and must outlive the table.  The column statistics gathered here (min / max, byte-value sets,
 * whether a column ascends) shape the kernels compiled against the table (dense group ids, key bitmaps, rank dictionaries), so
 * the CONTENT of adopted columns should not change while queries compiled over the table are in use.  If it does, nothing is
 * answered wrongly in silence: kernels over adopted columns check every value they derive from the statistics - a key outside
 * [min, max], a CHAR(1) / BOOL value that is not in the byte-value set (also one INSIDE the range: 'B' where the set was
 * {A, N, R}), two build rows with one key where the keys were unique - and the execution fails with RSQ_ERR_RUNTIME ("column
 * statistics"), or falls back to the general form of the table, instead of touching memory it should not or counting a row into a
 * neighbouring group.  (Columns the engine owns - uploaded, generated, loaded from '.tbl' - cannot change and skip those checks.)
 * After changing adopted data call rsq_table_refresh_stats and compile the statements anew. */
int  rsq_table_create_device(rsq_ctx* ctx, const rsq_table_desc* desc, rsq_table** out);
/* Gather the column statistics of `t` again (adopted columns whose content the host changed in place; the reference has no
 * counterpart - its operators take whatever values arrive, operators/aggregation.h:240-295).  Queries compiled BEFORE the call keep the
 * statistics they were compiled with (and their checks); compile the statement again to plan with the new ones. */
int  rsq_table_refresh_stats(rsq_table* t);
/* Transpose a ReSQL row store (reference src/dbdata.h: DataBlocks of packed tuples, strings by
 * value) into device columns: the bridge for a host that keeps ReSQL's own Relation objects.
 * The tuples are transposed where the context's rsq_ctx_set_rowstore_bridge says (the host by default): the call is
 * rsq_table_from_rowstore_ex with NULL options. */
int  rsq_table_from_rowstore(rsq_ctx* ctx, const rsq_table_desc* schema /* data pointers ignored */,
                             const uint8_t* const* blocks, const size_t* content_size, int32_t n_blocks,
                             rsq_table** out);
/* The same bridge with the transposition on the DEVICE (opt-in: rsq_ctx_set_rowstore_bridge, or mode 2 here).  The host path zero-fills
 * one buffer per column, walks every tuple on one thread and uploads the columns from pageable memory.  The device path copies the
 * tuples - whole tuples, packed back to back, chunk_bytes at a time - into one of two pinned buffers, sends the chunk to the device
 * behind the kernel of the chunk before it, and one kernel per chunk writes every cell of the chunk's rows into the columns
 * (resql_amd/csrc/rowstore.h holds the rule of a cell for both sides: a string's bytes behind its first NUL are zero in the column).
 * Columns, statistics and errors are those of the host path byte for byte.  Besides the columns the call holds two chunks of device
 * memory and two of pinned memory from the context's arenas, given back however it ends.  The call takes the host path - reported,
 * never an error - where the context has no device or the table has more than 64 columns.
 * Options and report carry struct_size like rsq_config: the library reads / writes no more than that many bytes. */
typedef struct rsq_rowstore_options {
    uint32_t struct_size;            /* sizeof(rsq_rowstore_options) */
    int32_t  mode;                   /* 0: the context's setting; 1: host; 2: device; else RSQ_ERR_INVALID */
    int64_t  chunk_bytes;            /* bytes of tuples per chunk (0: 64 MiB; raised to one tuple where smaller; < 0 or > 1 GiB: RSQ_ERR_INVALID) */
} rsq_rowstore_options;
enum rsq_rowstore_fallback { RSQ_ROWSTORE_FALLBACK_NONE = 0, RSQ_ROWSTORE_FALLBACK_NO_DEVICE = 1, RSQ_ROWSTORE_FALLBACK_COLUMNS = 2 };
typedef struct rsq_rowstore_report {
    uint32_t struct_size;            /* sizeof(rsq_rowstore_report) */
    int32_t  path;                   /* 0: transposed by the host; 1: on the device */
    int32_t  fallback_reason;        /* rsq_rowstore_fallback: why a call that asked for the device took the host path (0: it did not) */
    int32_t  reserved;
    int64_t  rows, tuple_bytes;      /* tuples taken from the blocks, and their bytes */
    int64_t  chunks;                 /* device path: chunks sent */
    /* host wall time in ms.  Device path: stage = the copies into the pinned buffers, copy = waiting for the link behind them,
     * kernel = HIP events around the kernels.  Host path: transpose = the host loop, copy = the upload of the columns. */
    double   stage_ms, copy_ms, kernel_ms, transpose_ms, stats_ms, total_ms;
} rsq_rowstore_report;
int  rsq_table_from_rowstore_ex(rsq_ctx* ctx, const rsq_table_desc* schema /* data pointers ignored */, const uint8_t* const* blocks,
                                const size_t* content_size, int32_t n_blocks, const rsq_rowstore_options* options /* NULL: the defaults */,
                                rsq_rowstore_report* report /* may be NULL */, rsq_table** out);
/* Where mode 0 - and so rsq_table_from_rowstore - transposes: 0 host (the default), 1 device; else RSQ_ERR_INVALID naming
 * "rowstore_bridge".  A setter, not a field: rsq_config keeps its size. */
int  rsq_ctx_set_rowstore_bridge(rsq_ctx* ctx, int32_t where);
/* BULK INSERT: load a '.tbl' text file (one tuple per line, fields ended by `field_terminator`, dbgen style with or
 * without the trailing terminator) straight into device columns, with the parsing rules of the reference's
 * executeBulkInsert / parseConstant (reference src/execute.h:332-388, src/expressions.h:369-515): see
 * resql_amd/csrc/tbl.cpp for the rules that matter (DECIMAL = digits with the point removed, BIGINT through int32,
 * dates as yyyy-mm-dd or yyyy/mm/dd).  `schema` gives names and types (data pointers ignored).
 * n_threads <= 0: all host threads.  Malformed lines give RSQ_ERR_INVALID with the line number.
 * The text is parsed where the context's rsq_config.tbl_ingest says: the call is rsq_table_load_tbl_ex with NULL options. */
int  rsq_table_load_tbl(rsq_ctx* ctx, const rsq_table_desc* schema, const char* path, char field_terminator,
                        int32_t n_threads, rsq_table** out);
/* The same load with the parse on the DEVICE (opt-in: rsq_config.tbl_ingest = 1, or mode 2 here).  The file is streamed into device
 * memory in chunk_bytes pieces through two pinned buffers; kernels find the lines and parse every line whose fields all have a PLAIN
 * form (resql_amd/csrc/tbl_fields.h: -?digits for INT / BIGINT, digits with at most one '.' for DECIMAL, dddd-dd-dd or dddd/dd/dd,
 * true / false, any text without NUL); every other line - leading blanks, signs, trailing garbage, a wrong field count - is parsed by
 * the host path's own line function and patched into the columns, so columns, statistics, error texts and line numbers are those of
 * the host path byte for byte.  The load takes the host path for the whole file - reported, never an error - where the context has
 * no device, the table has more than 64 columns, the terminator is '\n' or NUL, text + line offsets + columns exceed
 * max_device_text_bytes, or more than 65536 lines are not plain.
 * Options and report carry struct_size like rsq_config: the library reads / writes no more than that many bytes. */
typedef struct rsq_tbl_load_options {
    uint32_t struct_size;            /* sizeof(rsq_tbl_load_options) */
    int32_t  mode;                   /* 0: the context's tbl_ingest; 1: host; 2: device; else RSQ_ERR_INVALID */
    int64_t  chunk_bytes;            /* bytes per piece of the file on its way to the device (0: 64 MiB; 1..63 and < 0: RSQ_ERR_INVALID) */
    int64_t  max_device_text_bytes;  /* device memory the load may take while it runs (0: what is free minus 1 GiB; < 0: RSQ_ERR_INVALID) */
} rsq_tbl_load_options;
enum rsq_tbl_fallback { RSQ_TBL_FALLBACK_NONE = 0, RSQ_TBL_FALLBACK_NO_DEVICE = 1, RSQ_TBL_FALLBACK_COLUMNS = 2, RSQ_TBL_FALLBACK_TERMINATOR = 3,
                        RSQ_TBL_FALLBACK_DOES_NOT_FIT = 4, RSQ_TBL_FALLBACK_ODD_LINES = 5 };
typedef struct rsq_tbl_load_report {
    uint32_t struct_size;            /* sizeof(rsq_tbl_load_report) */
    int32_t  path;                   /* 0: parsed by host threads; 1: parsed on the device */
    int32_t  fallback_reason;        /* rsq_tbl_fallback: why a load that asked for the device took the host path (0: it did not) */
    int32_t  reserved;
    int64_t  rows, text_bytes;
    int64_t  lines_patched;          /* lines the host's line function parsed for the device path */
    /* host wall time in ms.  Device path: read = file reads into the pinned buffers, copy = waiting for the copies behind them,
     * kernel = HIP events around the three kernels, patch = the odd lines.  Host path: read = file read + parse, copy = upload. */
    double   read_ms, copy_ms, kernel_ms, patch_ms, stats_ms, total_ms;
    double   count_kernel_ms, starts_kernel_ms, parse_kernel_ms;     /* kernel_ms by kernel (HIP events), for measurements */
} rsq_tbl_load_report;
int  rsq_table_load_tbl_ex(rsq_ctx* ctx, const rsq_table_desc* schema, const char* path, char field_terminator, int32_t n_threads,
                           const rsq_tbl_load_options* options /* NULL: the defaults */, rsq_tbl_load_report* report /* may be NULL */,
                           rsq_table** out);
/* Fill a lineitem / orders / customer / synthetic table on the device with the deterministic
 * generator of resql_amd/datagen.py (same bits), rows [row0, row0 + n_rows).  kind: 0 lineitem,
 * 1 orders, 2 customer, 3 synthetic 4 x int64 (param = number of groups). */
int  rsq_table_generate(rsq_ctx* ctx, int32_t kind, int64_t row0, int64_t n_rows, double scale_factor,
                        int64_t param, uint64_t seed, rsq_table** out);
int64_t rsq_table_rows(const rsq_table* t);
/* BULK INSERT appends (executeBulkInsert adds tuples to the Relation it finds, reference src/execute.h:332-388; a Relation also grows
 * under its AppendIterator, src/dbdata.h:246-330): the rows of `more` - same context, same column types, made by any of the functions
 * above from the NEW tuples only - go behind the rows of `t`; `more` is consumed (destroyed) on success.  Column statistics are gathered
 * again and the columns move: a statement compiled BEFORE the call is refused afterwards (rsq_query_execute returns RSQ_ERR_INVALID,
 * "compile it again") - a ReSQL host compiles per statement anyway (execute.h:213-247). */
int  rsq_table_append(rsq_table* t, rsq_table* more);
/* A table that is a row range [row0, row0 + n_rows) of a larger one (a shard): rows are numbered from row0 wherever a row number
 * is observable — the order in which groups first occur decides the emission order of an aggregation (operators/aggregation.h:
 * 298-343 scans the hash table the groups entered in input order).  Set before queries are compiled over the table. */
int  rsq_table_set_first_row(rsq_table* t, int64_t row0);
/* Shards of ONE table must plan as that table.  The reference has one Relation and one hash table all its workers reach
 * (src/operators/aggregation.h:240-295, src/JitContextFlounder.h:459-487), so it never sees a "shard"; here the planner reads column
 * statistics (dense group ids come from a column's byte-value set or [min, max] range) and the row count (the reference sizes its
 * aggregation table from Relation::tupleNum(), which decides the emission order) of the table it is handed.  Before compiling
 * a plan over a shard, give it every shard's statistics: rsq_table_stats_export writes this table's fixed-size blob
 * (rsq_table_stats_bytes; the same size on every shard of a schema), the host moves the blobs (one all-gather between rank
 * processes), and rsq_table_unify_shard_stats(t, blobs of ALL shards incl. t's own, back to back) makes t plan with the union of the
 * value sets / ranges and the summed row count.  All shards then derive the same partial-table layout whatever their rows hold
 * (a shard without any 'R' row still keeps a cell for 'R'); where the union is not dense the plan takes the hash aggregation on
 * every shard alike.  rsq_multi_query_compile does this itself for the shards it is given.  rsq_table_total_rows: the summed count
 * (before unification: this table's own). */
int64_t rsq_table_stats_bytes(const rsq_table* t);
int  rsq_table_stats_export(const rsq_table* t, void* buf, int64_t bytes);
int  rsq_table_unify_shard_stats(rsq_table* t, const void* blobs, int32_t n_shards, int64_t blob_bytes);
int64_t rsq_table_total_rows(const rsq_table* t);
/* The dictionary counterpart, for shards that live in ONE process (on any contexts and devices): column by column over the n_shards
 * instances of a table (one schema, else RSQ_ERR_INVALID).  Where every shard with rows holds a dictionary image of the column and the
 * union of their entries has at most 256 values, every shard receives the union (bytewise order) and its codes are rewritten in place;
 * every other column stays exactly as it is.  A shard whose dictionary or codes changed refuses the statements compiled before, as after
 * rsq_table_append; shards that hold the union already are left alone, so a second call changes nothing.  rsq_multi_query_compile
 * calls it for every sharded table of a handle with RSQ_ENGINE_DICT_MULTI. */
int  rsq_table_unify_shard_dictionaries(rsq_table* const* shards, int32_t n_shards);
/* Measurement: the device time (ms) of one pass over a dictionary-coded column of a device table.  which 0: the recode pass that
 * installs a union (here under the identity map); which 1: encoding the wide column anew with the column's dictionary, which the recode
 * pass replaces.  The codes are left as they were. */
int  rsq_table_time_dictionary_pass(rsq_table* t, const char* column, int32_t which, double* ms);
/* Copy one device column back (tests). */
int  rsq_table_read_column(rsq_ctx* ctx, const rsq_table* t, const char* name, void* host_dst, size_t bytes);
void rsq_table_destroy(rsq_table* t);

/* ---- queries ----------------------------------------------------------------------------- */
/* tables[i] is the table SCAN operators refer to by index i. */
int  rsq_query_compile(rsq_ctx* ctx, const rsq_plan_desc* plan, rsq_table* const* tables, int32_t n_tables,
                       rsq_query** out);
/* Run all pipelines and finalise the result.  Blocking, like JitContextFlounder::execute(). */
int  rsq_query_execute(rsq_query* q);
/* Low compile latency (the reference compiles a query in 0.6-3 ms, src/JitContextFlounder.h:410-456): a plan whose specialised
 * kernels are not in the code-object cache is served by pre-compiled interpreter kernels from its first execution on - whole
 * pipelines: scans, selections, projections, join builds and probes, strings, dense / hash / at-the-join-entry aggregation,
 * materialisation - while hiprtc builds the kernels on host threads in two tiers (a quick one with stage 2 of a compacted
 * pipeline as a call, then the inlined one); an execution that finds a tier ready switches over.  Results are identical on
 * every tier.  rsq_query_await_kernels blocks until the query runs on its final kernels (benchmarks call it before timing);
 * it returns at once for queries that never were on the interpreter.  Environment: RSQ_GENERIC=0 compiles blocking,
 * RSQ_FORCE_GENERIC=1 keeps eligible plans on the interpreter (tests). */
int  rsq_query_await_kernels(rsq_query* q);
/* Multi-GPU (row-range sharded scans): run the pipelines up to the aggregation and stop.  The
 * dense partial aggregate table then sits in device memory at *dev_ptr as int64 words laid out
 * [ n_min_words | n_max_words | n_sum_words ]: the first segment merges with MIN (first-row
 * trackers, MIN aggregates), the second with MAX, the third with SUM (sums, counts) — one RCCL
 * all-reduce per non-empty segment, issued by the host (one process per GPU).
 * rsq_query_finalize then produces the result from the reduced table. */
int  rsq_query_execute_partial(rsq_query* q, void** dev_ptr, int64_t* n_min_words, int64_t* n_max_words,
                               int64_t* n_sum_words);
/* Same step without the host synchronisation: the pipelines are enqueued on the context's stream and the call
 * returns.  Work the caller enqueues on that stream afterwards (the merge collective over the bound partial table,
 * rsq_query_bind_partial) is ordered behind the kernels; rsq_query_finalize() synchronises once, checks the device
 * error word and fills the report.  Dense aggregations without join build pipelines only (everything else needs the
 * host between kernels); pair it with rsq_ctx_set_stream so that the caller's collectives share the stream. */
int  rsq_query_execute_partial_async(rsq_query* q);
/* Make the context launch on the caller's HIP stream (use_callers_stream != 0; hip_stream may be the null stream) or go
 * back to its own non-blocking stream (use_callers_stream == 0).  Synchronises the stream it leaves. */
int  rsq_ctx_set_stream(rsq_ctx* ctx, void* hip_stream, int32_t use_callers_stream);
int  rsq_query_finalize(rsq_query* q);
/* Same, from a partial aggregate table that is already in host memory (n_words int64 words in the
 * layout above).  Needs no device: it is the merge + finalisation step of the multi-GPU path in
 * isolation, which is how the CPU-only tests cover it (gloo). */
int  rsq_query_finalize_host(rsq_query* q, const int64_t* words, int64_t n_words);
/* Word counts of the partial aggregate table ([min | max | sum] segments), known after compile. */
int  rsq_query_partial_layout(const rsq_query* q, int64_t* n_min_words, int64_t* n_max_words, int64_t* n_sum_words);
/* Make the query keep its partial aggregate table in caller-owned device memory (e.g. a torch
 * tensor the host hands to RCCL) instead of its own allocation; `bytes` must cover all words. */
int  rsq_query_bind_partial(rsq_query* q, void* dev_ptr, size_t bytes);
/* The kernel behind the merge collective of small tables: `gathered_dev` holds the partial tables of `n_ranks` ranks back to
 * back (the receive buffer of ONE all-gather, device memory); they are reduced segment by segment (min | max | sum) into this
 * query's own partial table (the bound one).  Enqueued on the context's stream; no synchronisation. */
int  rsq_query_merge_gathered(rsq_query* q, const void* gathered_dev, int32_t n_ranks);
int  rsq_query_result(rsq_query* q, rsq_result_view* out);
int  rsq_query_report(const rsq_query* q, rsq_report* out);
/* Device time (HIP events around the launches) summed over the executions since the last reset, and their number: what a
 * benchmark loop reads ONCE after its timed region instead of a report per step (the reference prints executionTime per
 * query, JitContextFlounder.h:132-150; a loop of 50 steps would otherwise time its own bookkeeping). */
int  rsq_query_kernel_time_stats(rsq_query* q, double* sum_ms, uint64_t* executions, int32_t reset);
/* *out = S, the inner-range slices of the most recent execution's top nested-loops pipeline: 1 where it was not split (a materialising
 * pipeline, a small inner side, nested_loops_inner_slices = 1), 0 for a plan without such a join or before the first execution. */
int  rsq_query_nested_loops_slices(const rsq_query* q, int32_t* out);
/* The policy behind S, a pure function (no context, no device).  base_workgroups: the workgroups the outer side's tiles ask for;
 * max_workgroups: the most this pipeline launches (workgroups per CU x CUs, scaled by the block size, clamped to what is resident);
 * configured: rsq_config.nested_loops_inner_slices.
 *   configured == 1 -> 1;  configured >= 2 -> min(configured, max_workgroups);
 *   configured == 0 -> max(1, min(max_workgroups / base_workgroups, ceil(inner_rows / RSQ_NLJ_MIN_SLICE_ROWS)))
 * The launch then has S x max(1, min(base_workgroups, max_workgroups / S)) workgroups. */
#define RSQ_NLJ_MIN_SLICE_ROWS 512     /* fewest inner rows worth a slice of their own: it re-reads the outer rows and flushes its own partial result */
int32_t rsq_nested_loops_slices(int64_t base_workgroups, int64_t max_workgroups, int64_t inner_rows, int32_t configured);
/* Generated HIP source and pipeline description of the compiled query (debugging). */
const char* rsq_query_source(const rsq_query* q);
const char* rsq_query_explain(const rsq_query* q);
void rsq_query_destroy(rsq_query* q);

/* ---- host-side helpers that mirror reference free functions ------------------------------ */
/* serializeExpr after deriveExpressionTypes (reference src/expressions.h:177-204, 1367-1392): lets a
 * host check the engine's typing against the reference's (test/test_datatypes.h).  Returns a
 * malloc'ed string (free with rsq_free) or NULL. */
char* rsq_serialize_expr(rsq_ctx* ctx, const rsq_plan_desc* plan, int32_t expr, int32_t derive,
                         rsq_table* const* tables, int32_t n_tables);
/* serializeRelation (reference src/dbdata.h:688-701) of a result view. */
char* rsq_result_serialize(const rsq_result_view* view);
void  rsq_free(void* p);
/* The same text of a query's result, optionally written on the DEVICE (opt-in: rsq_ctx_set_result_text, or mode 2 here).  The host
 * path is rsq_result_serialize's: one thread, one cell after the other, and it stays the definition of the text.  The device path
 * produces the same bytes: the tuples are uploaded in chunks of chunk_rows rows, one kernel takes every row's text length (one lane
 * per row; resql_amd/csrc/result_text.h holds the text of a cell for both sides), the toolkit's exclusive scan turns the workgroups'
 * totals into offsets, a second kernel writes the text - staged in LDS and stored 16 bytes per lane where a workgroup's span fits
 * the tile - and the text comes back through pinned staging.  Device and pinned memory are the context's arenas' and are given back
 * however the call ends.  The call takes the host path - reported, never an error - where the context has no device, the schema
 * is outside the device form (more than 64 columns, CHAR of length 0, a DECIMAL scale above 18, a row whose text may exceed
 * 64 KiB), or a chunk of one row does not fit max_device_bytes.  Where the materialisation's device tail (rsq_ctx_set_result_pack)
 * made the result and no ORDER BY reordered it on the host, or the device sort (rsq_ctx_set_order_sort) delivered it in the ORDER BY's
 * order, the kernels read the tuples in the query's own device buffer, chunk by
 * chunk at any byte offset: no tuple buffer is allocated, nothing is uploaded, tuples_from_device is 1 and upload_ms 0.  That buffer is
 * the query's from the execution until its next execution or its destruction, whatever other statements run in between.  Every other
 * result - the aggregation tails' among them, whose arena space is not the query's to keep - is uploaded from the host copy the result
 * view hands out (tuples_from_device 0).
 * Options and report carry struct_size like rsq_config: the library reads / writes no more than that many bytes.  A query that has
 * not been executed answers as rsq_query_result does (a relation of no rows).  The handles of several GPUs keep the host text. */
typedef struct rsq_result_text_options {
    uint32_t struct_size;            /* sizeof(rsq_result_text_options) */
    int32_t  mode;                   /* 0: the context's setting; 1: host; 2: device; else RSQ_ERR_INVALID */
    int64_t  chunk_rows;             /* rows per chunk (0: chosen, so that a chunk's text stays below 2^32 bytes and within the budget; < 0: RSQ_ERR_INVALID) */
    int64_t  max_device_bytes;       /* device memory the call may take while it runs (0: what is free minus 1 GiB; < 0: RSQ_ERR_INVALID) */
} rsq_result_text_options;
enum rsq_text_fallback { RSQ_TEXT_FALLBACK_NONE = 0, RSQ_TEXT_FALLBACK_NO_DEVICE = 1, RSQ_TEXT_FALLBACK_SCHEMA = 2, RSQ_TEXT_FALLBACK_DOES_NOT_FIT = 3 };
typedef struct rsq_result_text_report {
    uint32_t struct_size;            /* sizeof(rsq_result_text_report) */
    int32_t  path;                   /* 0: written by the host; 1: on the device */
    int32_t  fallback_reason;        /* rsq_text_fallback: why a call that asked for the device took the host path (0: it did not) */
    int32_t  tuples_from_device;     /* 1: the kernels read the tuples where a device tail had left them; 0: uploaded from the host */
    int64_t  rows, text_bytes, chunks;
    /* ms.  Device path: HIP events around the uploads, the kernels (lengths, scan, write) and the copies back; download_ms also
     * holds the host's copy out of the staging buffer (or its fwrite).  Host path: total_ms alone. */
    double   upload_ms, kernel_ms, download_ms, total_ms;
} rsq_result_text_report;
/* *text: malloc'ed, *text_bytes long and NUL-terminated behind that (rsq_free). */
int  rsq_query_result_text(rsq_query* q, const rsq_result_text_options* options /* NULL: the defaults */, rsq_result_text_report* report /* may be NULL */,
                           char** text, int64_t* text_bytes);
/* ... straight into the file `path` (created or truncated) */
int  rsq_query_result_write(rsq_query* q, const char* path, const rsq_result_text_options* options, rsq_result_text_report* report);
/* Where mode 0 and the statement loop's `tofile` write their text: 0 host (the default), 1 device; else RSQ_ERR_INVALID naming
 * "result_text".  A setter, not a field: rsq_config keeps its size. */
int  rsq_ctx_set_result_text(rsq_ctx* ctx, int32_t where);
/* The register aggregation's second form.  A register aggregation with 32-bit partial sums that runs four waves per SIMD (TPC-H Q1) has a
 * second form of its kernel, in which every row adds its inputs into its lane's words of the workgroup's LDS image.  mode -1 (the
 * default): a statement runs each form in two timed executions and keeps the second only where its kernel time is clearly the better
 * one; 0: statements compiled from now on get no second form (the kernel text of earlier versions); 1: they run it in every launch
 * that fits the fields of its shared words.  The answers are the same bit for bit.  Read when a statement is compiled (under 0 it
 * gets no second form at all) and at every launch: 0 or 1 set later holds from the next execution on, for compiled statements too
 * (0 then runs form 0 of the two-form text, whatever the statement had measured or the plan memo remembered). */
int  rsq_ctx_set_row_cells(rsq_ctx* ctx, int32_t mode);
/* ORDER BY ... LIMIT k over a materialisation (a plan without an aggregation whose root is an ORDER BY with a LIMIT), optionally
 * decided from rows the DEVICE selects (opt-in: rsq_ctx_set_order_limit).  The host path copies every column of every materialised row
 * to the host, packs tuples, runs the reference's quicksort over all of them and drops what lies behind row k; it stays the definition
 * of the answer.  The device path rests on the rule the aggregation tails use: the k first rows of the reference's sorted order are
 * determined by the sort keys alone unless rows among the leading k + 1 tie on ALL keys.  With want = k + 1, it finds T, the want-th
 * largest image of the first key (resql_amd/csrc/order_limit.h: key ^ 2^63, complemented for ascending order, the cell read at its own
 * width) by an MSB-first radix select over the key's column, takes the candidates - every row with image >= T, in SCAN ORDER: one count
 * per 256-row block, the toolkit's exclusive scan, a gather by ballot ranks - and writes their scan positions and their cells of every
 * materialised column (numbers at their width, strings as spans of their column width) into compact columns of at most
 * capacity = max(4 * want, 65536) rows.  Only those come back, through pinned memory; the host packs them into tuples with the function
 * the full path packs all rows with, partial-sorts the leading want of them by the full key list, and - where every adjacent pair of
 * those is strictly ordered - the first min(k, rows) are the result relation.  The full path runs, over the columns that are still on
 * the device, where the report says so: FEW_ROWS 4 * k >= rows, OVERFLOW more candidates than capacity (many rows share the first
 * key's leading value), TIES, and SHAPE: the plan is not eligible (an aggregation, no LIMIT, a LIMIT beyond 2^20, a LIMIT on the
 * materialisation itself, a first key that is not a materialised INT / DATE / BIGINT / DECIMAL attribute, more than 32 columns) or the
 * execution is not (a shard of rsq_multi_*, rsq_query_execute_partial).  0: host (the default - the launches and bytes of earlier
 * versions), 1: device; else RSQ_ERR_INVALID naming "order_limit".  A setter, not a field: rsq_config keeps its size.  Read at every
 * execution: it holds for statements compiled earlier too.  The device and pinned buffers are the context's arenas', kept by the
 * query between executions and given back with it. */
int  rsq_ctx_set_order_limit(rsq_ctx* ctx, int32_t where);
enum rsq_order_limit_fallback { RSQ_ORDER_LIMIT_FALLBACK_NONE = 0, RSQ_ORDER_LIMIT_FALLBACK_SHAPE = 1, RSQ_ORDER_LIMIT_FALLBACK_FEW_ROWS = 2,
                                RSQ_ORDER_LIMIT_FALLBACK_OVERFLOW = 3, RSQ_ORDER_LIMIT_FALLBACK_TIES = 4 };
typedef struct rsq_order_limit_report {
    uint32_t struct_size;            /* sizeof(rsq_order_limit_report), set by the caller: no more than that many bytes are written */
    int32_t  planned;                /* 1: the compiled plan is of the eligible shape (known after compile, also on a compile-only context) */
    int32_t  path;                   /* of the last execution - 0: the host sorted everything; 1: decided from device-selected candidates */
    int32_t  fallback_reason;        /* rsq_order_limit_fallback: why an execution under setting 1 took the host path (0: it did not) */
    int32_t  first_key_column;       /* planned: the materialised column the first ORDER BY expression names (else -1) */
    int32_t  key_is32;               /* ... compared as signed 32 bits (INT, DATE); 0: as signed 64 bits (BIGINT, DECIMAL) */
    int32_t  descending;             /* ... DESC */
    int32_t  reserved;
    int64_t  rows, want, candidates, capacity;      /* materialised rows, k + 1, rows with image >= T (exact, also above capacity), candidate rows the buffers hold */
    /* ms.  select_ms: HIP events around the selection and gather kernels; copy_ms: the host's wait for the candidate count and the
     * copy of positions and candidate columns; tail_ms: tuples, partial sort, tie check (on the host path: 0 - rsq_report.finalize_time_ms) */
    double   select_ms, copy_ms, tail_ms;
} rsq_order_limit_report;
int  rsq_query_order_limit_report(const rsq_query* q, rsq_order_limit_report* out);
/* The result tuples of a materialisation (a plan without an aggregation: every SELECT of columns), optionally packed on the DEVICE
 * (opt-in: rsq_ctx_set_result_pack).  The host path copies every output column to the host on its own, zero-fills the relation and
 * packs ReSQL tuples on the worker pool; it stays the definition of the bytes.  The device path packs all rows in one launch
 * (resql_amd/csrc/result_pack.h holds the bytes of a field for both sides: a number's cell, CHAR(1)'s byte and a zero, a string cut at
 * its first NUL with zeros behind it - every byte of every tuple is written), copies the tuples once into pinned memory, which the
 * result view then hands out, and keeps them on the device for rsq_query_result_text / _write and `tofile`.  An ORDER BY above the
 * materialisation that rsq_ctx_set_order_limit did not decide runs the reference's quicksort over the pinned tuples in place
 * (sorted_on_host; the device's copy is then not in the result's order and is not read).  An execution under setting 1 takes the host
 * path - reported, never an error - for SHAPE: an aggregation, no materialisation, more than 64 materialised columns, a shard of
 * rsq_multi_*, rsq_query_execute_partial, a sub-query's own execution (a nested-loops inner side, a derived table); SMALL: no rows,
 * or output columns in host-mapped memory (results of up to 256 KB of cells per column: the host has them already); DOES_NOT_FIT:
 * 2^32 rows or more, rows x tuple size above 2 GiB (rpack::MAX_TUPLE_BYTES), or that many bytes not free on the device with 1 GiB to
 * spare; ORDER_LIMIT: rsq_ctx_set_order_limit decided the answer from its candidates and no materialised row was packed at all.
 * 0: host (the default - the launches, copies and bytes of earlier versions), 1: device; else RSQ_ERR_INVALID naming "result_pack".
 * A setter, not a field: rsq_config keeps its size.  Read at every execution: it holds for statements compiled earlier too.  The
 * device and pinned buffers are the context's arenas', kept by the query between executions, grown on demand and given back with it
 * and not before: a query that has run under setting 1 keeps them (up to 2 GiB each) beside the host path's buffers while later
 * executions run under setting 0 or fall back. */
int  rsq_ctx_set_result_pack(rsq_ctx* ctx, int32_t where);
enum rsq_result_pack_fallback { RSQ_RESULT_PACK_FALLBACK_NONE = 0, RSQ_RESULT_PACK_FALLBACK_SHAPE = 1, RSQ_RESULT_PACK_FALLBACK_SMALL = 2,
                                RSQ_RESULT_PACK_FALLBACK_DOES_NOT_FIT = 3, RSQ_RESULT_PACK_FALLBACK_ORDER_LIMIT = 4 };
typedef struct rsq_result_pack_report {
    uint32_t struct_size;            /* sizeof(rsq_result_pack_report), set by the caller: no more than that many bytes are written */
    int32_t  planned;                /* 1: the compiled plan is of the eligible shape (known after compile, also on a compile-only context) */
    int32_t  path;                   /* of the last execution - 0: the host packed the tuples; 1: the device did */
    int32_t  fallback_reason;        /* rsq_result_pack_fallback: why an execution under setting 1 took the host path (0: it did not) */
    int32_t  sorted_on_host;         /* 1: an ORDER BY above the materialisation ran the reference's quicksort over the delivered tuples */
    int32_t  tuple_size;             /* the packed relation: bytes per tuple, ... */
    int64_t  rows, tuple_bytes;      /* ... its rows (behind ORDER BY's LIMIT) and rows x tuple_size (planned shapes; else 0) */
    /* ms, device path.  kernel_ms: HIP events around the pack kernel; copy_ms: the host's wait and the copy of the tuples; sort_ms: the host's sort */
    double   kernel_ms, copy_ms, sort_ms;
} rsq_result_pack_report;
int  rsq_query_result_pack_report(const rsq_query* q, rsq_result_pack_report* out);
/* ORDER BY over a materialisation (a plan without an aggregation whose root is an ORDER BY directly above the MATERIALIZE, with any
 * LIMIT or none), optionally sorted on the DEVICE (opt-in: rsq_ctx_set_order_sort).  The host path packs every materialised row into a
 * tuple and runs the reference's quicksort over all of them on one thread; it stays the definition of the answer.  The device path
 * rests on the rule the aggregation tails and rsq_ctx_set_order_limit use: the reference's sorted order is determined by the sort keys
 * alone wherever no two adjacent rows of it tie on ALL keys.  Every key's cell becomes an image in which "earlier" is "smaller"
 * (resql_amd/csrc/order_sort.h: the complement of order_limit.h's image, the cell read at its own width); one pass finds every key's
 * least and greatest image; key j then takes 64 - clz(max_j - min_j) bits, the keys' (image - min) are concatenated, first key most
 * significant, and the string is cut into 64-bit words from its least significant end; the rows are ordered by a stable LSD radix sort
 * over the words (8 bits a pass, only the bits a word holds), so the device's order is "keys, then scan order"; a kernel counts the
 * positions among the leading `lead` rows - all rows without a LIMIT, min(rows, k + 1) with LIMIT k - whose row and successor are equal
 * on every key; all rows are packed into tuples in scan order (the kernel of rsq_ctx_set_result_pack, whatever that setting says) and
 * the leading out_rows = min(rows, k) tuples are gathered in the order into a device buffer the query keeps, copied once into pinned
 * memory, which the result view hands out, and read in place by rsq_query_result_text / _write and `tofile` (tuples_from_device 1).
 * An execution under setting 1 takes the host path - reported, never an error, the materialised columns untouched - for SHAPE: the
 * plan is not eligible (an aggregation, no ORDER BY at the root directly above the materialisation, a LIMIT on the materialisation
 * itself, no key or more than 8, a key that is not a materialised INT / DATE / BIGINT / DECIMAL attribute - strings, CHAR(1) and BOOL
 * compare by rules that are not a byte order -, more than 64 materialised columns) or the execution is not (a shard of rsq_multi_*,
 * rsq_query_execute_partial, a sub-query's own execution); SMALL: no rows, or output columns in host-mapped memory; DOES_NOT_FIT:
 * 2^32 rows or more, rows x tuple size above 2 GiB, or the sort's and the tuples' buffers not free on the device with 1 GiB to spare
 * (order_sort.h fitsDevice, asked before anything is allocated); TIES: tied_pairs > 0 - the passes have been paid and the host's
 * quicksort over all tuples follows, through rsq_ctx_set_result_pack where that is set; ORDER_LIMIT: rsq_ctx_set_order_limit decided the
 * answer first (where it fell back - FEW_ROWS, OVERFLOW, TIES, a LIMIT above 2^20 - this path runs next).
 * 0: host (the default - the launches, copies and bytes of earlier versions), 1: device; else RSQ_ERR_INVALID naming "order_sort".
 * A setter, not a field: rsq_config keeps its size.  Read at every execution: it holds for statements compiled earlier too.  The
 * device and pinned buffers are the context's arenas', kept by the query between executions, grown on demand and given back with it. */
int  rsq_ctx_set_order_sort(rsq_ctx* ctx, int32_t where);
enum rsq_order_sort_fallback { RSQ_ORDER_SORT_FALLBACK_NONE = 0, RSQ_ORDER_SORT_FALLBACK_SHAPE = 1, RSQ_ORDER_SORT_FALLBACK_SMALL = 2,
                               RSQ_ORDER_SORT_FALLBACK_DOES_NOT_FIT = 3, RSQ_ORDER_SORT_FALLBACK_TIES = 4, RSQ_ORDER_SORT_FALLBACK_ORDER_LIMIT = 5 };
typedef struct rsq_order_sort_report {
    uint32_t struct_size;            /* sizeof(rsq_order_sort_report), set by the caller: no more than that many bytes are written */
    int32_t  planned;                /* 1: the compiled plan is of the eligible shape (known after compile, also on a compile-only context) */
    int32_t  path;                   /* of the last execution - 0: the host sorted the tuples; 1: the device ordered the rows */
    int32_t  fallback_reason;        /* rsq_order_sort_fallback: why an execution under setting 1 took the host path (0: it did not) */
    int32_t  keys;                   /* planned: the ORDER BY's keys (else 0) */
    int32_t  key_bits[8];            /* of the last device sort: bits key j takes in the composite key (0: it does not vary) */
    int32_t  total_bits, words, passes;      /* ... their sum, its 64-bit words, the 8-bit radix passes taken */
    int32_t  tuple_size;             /* bytes per tuple of the materialised relation */
    int32_t  reserved;
    int64_t  rows, lead, out_rows;   /* materialised rows; leading rows checked for ties; rows of the result relation */
    int64_t  tied_pairs;             /* positions i, i + 1 < lead, whose rows are equal on every key */
    /* ms, device path.  range_ms, sort_ms (key words, passes, tie count), pack_ms, gather_ms: HIP events around the kernels; copy_ms: the
     * host's wait and the copy of the tuples */
    double   range_ms, sort_ms, pack_ms, gather_ms, copy_ms;
} rsq_order_sort_report;
int  rsq_query_order_sort_report(const rsq_query* q, rsq_order_sort_report* out);
/* The slot order of the reference's aggregation hash table (allocateHashTable / ht_put / growHashTable, src/qlib/hash.h:225-287,
 * 330-419) after inserting n groups with the given Values::hash values in this order into a table allocated for min_size
 * entries: out[k] = index of the group in the k-th occupied slot.  parallel != 0 takes the cluster-parallel replay the engine's
 * tail uses for many groups, 0 the sequential one; both give the same permutation (tests compare them). */
int   rsq_ref_emission_order(const uint64_t* hashes, int64_t n, uint64_t min_size, int32_t parallel, uint32_t* out);
/* The same on the GPU of `ctx` (the form the tail of a large dense aggregation uses): hashes and the result travel through device
 * memory.  RSQ_ERR_UNSUPPORTED for tables beyond the device path's range (2^31 slots). */
int   rsq_ref_emission_order_device(rsq_ctx* ctx, const uint64_t* hashes, int64_t n, uint64_t min_size, uint32_t* out);

/* ---- device primitives exposed for tests ---------------------------------------------------
 * The engine's exact integer kernels (aot_kernels.hip) run on the caller's data, so that a test reaches their chunk, sub-block, wave and
 * word boundaries with a few megabytes instead of the tables that reach them through a query.  Every pointer is host memory.  A call takes
 * its device buffers from the context's allocator, runs on the context's stream, waits for it, copies the result back and frees the
 * buffers.  *notes receives the bits of the device error word the call raised (64: the placement's record count is not the number of
 * distinct keys or exceeds the capacity; 128 / 512: a look-back of the one-launch rank index / scan gave up and the result is void); the
 * call clears them again, so the context stays usable.  RSQ_ERR_UNSUPPORTED on a context without a device, RSQ_ERR_INVALID for null
 * pointers, negative sizes and shapes the kernels would read or write out of bounds with. */
/* offsets[i] = counts[0] + ... + counts[i - 1] in 64 bits.  form 0: exclusiveScanCounts (three launches), 1: exclusiveScanCountsChained
 * (one launch, decoupled look-back). */
int   rsq_prim_exclusive_scan(rsq_ctx* ctx, const uint32_t* counts, int64_t n, int32_t form, uint64_t* offsets /* [n] */, uint32_t* notes);
/* The rank index of a key bitmap of n_blocks 32-byte blocks [rank word | 7 bitmap words]: word 0 of every block comes back as the number
 * of bits set in the bitmap words of the blocks before it, words 1..7 as they were; chunk_base[c] is the rank at block
 * c * 1024 and chunk_base[n_chunks] the number of bits set.  form 0: rankTableIndex (two launches), 1: rankTableIndexChained (one
 * launch; at most 1171 chunks). */
int   rsq_prim_rank_index(rsq_ctx* ctx, uint32_t* blocks /* [n_blocks * 8], in and out */, int64_t n_blocks, int32_t form,
                          uint32_t* chunk_base /* [ceil(n_blocks / 1024) + 1] */, uint32_t* notes);
/* rankTablePlace: the blocks are indexed (form 0), the record counter is the sum of used[], and every record - n_words words, word 0 its
 * key, used[w] of them at records[w * region * n_words] - is written to words_out at the rank of its key: the number of bits set below
 * bit (key - bm_min), which lives in bit d & 31 of word 1 + (d >> 5) % 7 of block (d >> 5) / 7.  words_out is filled with 0xff bytes
 * before the launch.  A record whose key lies outside [bm_min, bm_min + bm_bits) is skipped.  Requires bm_bits <= n_blocks * 224 and
 * used[w] <= region. */
int   rsq_prim_rank_place(rsq_ctx* ctx, const uint32_t* blocks /* [n_blocks * 8] */, int64_t n_blocks, int64_t bm_min, int64_t bm_bits,
                          const int64_t* records /* [n_waves * region * n_words] */, const uint32_t* used /* [n_waves] */, int32_t n_waves,
                          int32_t region, int32_t n_words, int64_t capacity, int64_t* words_out /* [capacity * n_words] */, uint32_t* notes);
/* The kernels that finish an aggregation (devtail.hip, aot_kernels.hip), under the same conventions.  None of them raises a bit of the error
 * word on the inputs these entry points accept, except the merge's 2 ("Hash table full"), which its table of >= 2 n slots does not reach. */
/* radixSortPairs: the pairs sorted, stably, by the low 8 * ceil(key_bits / 8) bits of their keys (whole 8-bit digits); key_bits 1..64.  The
 * result is copied from whichever of the two buffer pairs holds it; with n <= 1 nothing runs and the input is the answer. */
int   rsq_prim_radix_sort_pairs(rsq_ctx* ctx, const uint64_t* keys /* [n] */, const uint32_t* vals /* [n] */, int64_t n, int32_t key_bits,
                                uint64_t* keys_out /* [n] */, uint32_t* vals_out /* [n] */, uint32_t* notes);
/* out[i] = min(in[0..i]): the running minimum of the device replay of the reference's hash table (k_scanmin_chunks / _totals / _apply,
 * built on the scan toolkit of resql_amd/csrc/scan_device.h). */
int   rsq_prim_running_min(rsq_ctx* ctx, const int64_t* in /* [n] */, int64_t n, int64_t* out /* [n] */, uint32_t* notes);
/* mergeGroupRows: n group rows [first row | n_tab table words | accumulators] of `stride` words merged by key.  Key k is row word
 * key_word[k] of type key_type[k] (rsq_type_tag); key_len[k] is 0 for a number, 1 for CHAR(1), the declared length for CHAR(n) /
 * VARCHAR(n), whose bytes fill ceil(len / 8) consecutive words.  INT / DATE compare by their low 32 bits, BOOL / CHAR(1) by their low byte,
 * CHAR(n) without trailing spaces, VARCHAR up to its NUL.  Accumulator w is row word acc_word[w], merged by acc_kind[w]: 0 wrapping int64 sum,
 * 2 min, 3 max.  out_rows receives one row per group - first row: the members' minimum; table words: those of the member with that
 * first row; accumulators merged - in the order of the groups' owners (the member that claimed the group's slot), *out_count the number
 * of groups; the rows behind them are 0xff bytes.  Requires n < 2^31, n_keys <= 16, n_acc <= 32, every key inside words 1..n_tab, every
 * accumulator word inside n_tab + 1..stride - 1. */
int   rsq_prim_merge_group_rows(rsq_ctx* ctx, const int64_t* rows /* [n * stride] */, int64_t n, int32_t stride, int32_t n_tab,
                                const int32_t* key_word, const int32_t* key_type, const int32_t* key_len, int32_t n_keys, const int32_t* acc_word,
                                const int32_t* acc_kind, int32_t n_acc, int64_t* out_rows /* [n * stride] */, uint64_t* out_count, uint32_t* notes);
/* The ORDER BY ... LIMIT pre-selection over rows of `stride` words with the sort key in word key_word (is32: its low 32 bits, signed; desc:
 * larger first).  A key's image is (key ^ 2^63), complemented for ascending order, so "earlier in the order" is "larger".  n_rows goes
 * into a device word, as the engine's row count does; the kernels take min(n_rows, rows_upper_bound) rows.  form 0: selectTopCandidates,
 * the rows whose image is at or above the want-th largest.  form 1: prepareTopCandidatesRange, image_range = {largest image, ~smallest
 * image} copied into the scratch (the caller supplies it: nothing is computed here), selectTopCandidatesRange: the rows of the 11-bit bin
 * of the want-th largest image and of every bin above.  *cand_count is the number of such rows, cand_out - 0xff bytes before the launch -
 * holds the first `capacity` of them in no particular order.  Requires want >= 1, capacity >= 1, stride 1..64, key_word < stride. */
int   rsq_prim_topk_select(rsq_ctx* ctx, const int64_t* rows /* [n_rows * stride] */, int64_t n_rows, int64_t rows_upper_bound, int32_t stride,
                           int32_t key_word, int32_t is32, int32_t desc, int64_t want, int32_t form, const uint64_t* image_range /* [2], form 1 */,
                           int64_t capacity, int64_t* cand_out /* [capacity * stride] */, uint32_t* cand_count, uint32_t* notes);
/* The same pre-selection over a COLUMN, as ORDER BY ... LIMIT over a materialisation runs it (order_limit.hip, rsq_ctx_set_order_limit):
 * n keys of key_width 4 (signed 32 bits, sign-extended) or 8 bytes; *threshold_image receives T, the want-th largest image (0 where
 * n < want: every row is a candidate); *cand_count the number of rows with image >= T, exact also above capacity; positions_out
 * [capacity] their row numbers in ascending order and payload_out [capacity * payload_width] those rows' cells of the one payload column
 * (payload_width 1..4096 bytes per row, any value: the gather's byte path), both 0xff bytes before the launch and behind the first
 * min(count, capacity) candidates.  Requires 0 <= n < 2^32, want >= 1, 1 <= capacity < 2^31. */
int   rsq_prim_column_topk(rsq_ctx* ctx, const void* key /* [n * key_width] */, int32_t key_width, int64_t n, int32_t desc, int64_t want,
                           int64_t capacity, const void* payload /* [n * payload_width] */, int32_t payload_width,
                           uint32_t* positions_out /* [capacity] */, void* payload_out /* [capacity * payload_width] */, uint64_t* cand_count,
                           uint64_t* threshold_image, uint32_t* notes);
/* The materialisation's device tail over host columns (result_pack.hip, rsq_ctx_set_result_pack): columns[c] holds n_rows cells of
 * types[c] at the column's width (BOOL / CHAR(1) 1, INT / DATE 4, BIGINT / DECIMAL 8, CHAR(n) / VARCHAR(n) n bytes); each is uploaded
 * into a device buffer that ends with its last cell, and the kernel packs the tuples into a device buffer of n_rows x tuple size + 64
 * bytes filled with 0xEE before the launch.  out receives all of it, the 64 guard bytes included: out_bytes must be exactly that.
 * 1 to 64 columns, 0 <= n_rows < 2^31, at most 2 GiB of tuples. */
int   rsq_prim_pack_tuples(rsq_ctx* ctx, const void* const* columns, const rsq_type* types, int32_t n_cols, int64_t n_rows, void* out, int64_t out_bytes);
/* The device's order of column-wise rows (order_sort.hip, rsq_ctx_set_order_sort): columns[c] holds n_rows cells of types[c] at the
 * column's width; key_columns[j] names the j-th sort key, an INT / DATE / BIGINT / DECIMAL column, descending[j] != 0 its direction;
 * 1 to 8 keys.  perm_out[i] = the row that is i-th by "keys, then scan order"; *tied_pairs = the positions i, i + 1 < lead, whose rows
 * are equal on every key; key_bits[j] the bits key j takes in the composite key (8 entries are written), *words its 64-bit words.  Where
 * no key varies and lead > 1 nothing is sorted: the identity and lead - 1.  0 <= lead <= n_rows < 2^31. */
int   rsq_prim_sort_rows(rsq_ctx* ctx, const void* const* columns, const rsq_type* types, int32_t n_cols, const int32_t* key_columns,
                         const int32_t* descending, int32_t n_keys, int64_t n_rows, int64_t lead, uint32_t* perm_out /* [n_rows] */,
                         int64_t* tied_pairs, int32_t* key_bits /* [8] */, int32_t* words);
/* out tuple i = tuple perm[i] of `tuples` (n_rows tuples of tuple_size bytes) for i < n_out (order_sort.hip k_os_gather_tuples); every
 * perm[i] must be below n_rows.  The device's output buffer holds n_out x tuple_size + 64 bytes filled with 0xEE before the launch; out
 * receives all of it, the 64 guard bytes included: out_bytes must be exactly that.  0 <= n_out <= n_rows < 2^31, at most 2 GiB of tuples. */
int   rsq_prim_gather_tuples(rsq_ctx* ctx, const void* tuples, int32_t tuple_size, int64_t n_rows, const uint32_t* perm, int64_t n_out,
                             void* out, int64_t out_bytes);
/* What the statistics pass left beside a column (aot_kernels.hip computeColumnStats), copied back as it lies: which 0 the narrow image
 * (rows values of `width` bytes, each the row's value minus `base`), 1 the dictionary's entries (as many as the column has, each as wide as
 * the column, in memcmp order), 2 the dictionary codes (one byte per row).  info = {width in bytes (0: no narrow image), base, dictionary
 * entries (0: no dictionary), rows} is filled whatever `which` and `bytes` are; with bytes == 0 nothing else happens.  No kernel runs and
 * no state changes.  RSQ_ERR_INVALID for null pointers, a `which` outside 0..2, an unknown column and a read beyond rows * width,
 * entries * column width or rows.  A compile-only context has no images: which 0 and 2 with bytes > 0 are RSQ_ERR_UNSUPPORTED there, and
 * which 1 is the host's copy of the entries. */
int   rsq_table_read_image(rsq_ctx* ctx, const rsq_table* t, const char* column, int32_t which, void* host_dst, size_t bytes, int64_t info[4]);

/* ---- SQL text in front of the path --------------------------------------
 * The reference turns SQL text into an operator tree with parseSql (src/parser/parseSql.h:130-166:
 * tokens of src/parser/lexer.y, grammar of src/parser/parser.y) and buildQuery (src/planner.h:409-497),
 * then calls executeSelectPlan (src/execute.h:213-247) — the boundary above.  These entry points are
 * that front end for a host that has no ReSQL planner of its own: the same tokens, grammar, desugaring
 * (BETWEEN, IN, CASE) and planning rules, producing the plan description of resql_plan.h.
 *
 * `tables` is the database: every table a FROM clause may name (rsq_table carries name, schema and
 * row count — what Database::relations holds, src/dbdata.h).  Scan operators of the plan index into it,
 * so the same array goes to rsq_query_compile.  Errors: RSQ_ERR_INVALID "Syntax error." (execute.h:520-523),
 * "Table x does not exist." (planner.h:437-439); RSQ_ERR_UNSUPPORTED for plans that need a nested-loops join, unless the context
 * has RSQ_ENGINE_NESTED_LOOPS (the pieces are then folded left-deep into RSQ_OP_NESTEDLOOPSJOIN nodes, as planner.h:458-469 does). */
typedef struct rsq_sql_plan rsq_sql_plan;
int  rsq_sql_plan_select(rsq_ctx* ctx, const char* sql, rsq_table* const* tables, int32_t n_tables, rsq_sql_plan** out);
const rsq_plan_desc* rsq_sql_plan_desc(const rsq_sql_plan* plan);
void rsq_sql_plan_destroy(rsq_sql_plan* plan);
/* the operator tree as text (what `showplan` prints in spirit; tests compare it with the reference's planner);
 * malloc'ed, rsq_free.  The tables passed to rsq_sql_plan_select must still be alive. */
char* rsq_sql_plan_text(const rsq_sql_plan* plan);
/* parse + plan + rsq_query_compile in one call (executeSelect, src/execute.h:250-260, up to ctx.compile()) */
int  rsq_sql_compile(rsq_ctx* ctx, const char* sql, rsq_table* const* tables, int32_t n_tables, rsq_query** out);
/* The statement as text, for hosts that dispatch on its kind (executeStatement, src/execute.h:508-545) and for
 * tests: what = 0 the token names one per line ("NAME text"), what = 1 the parsed statement ("SELECT" with its
 * clause expressions, "CREATE_TABLE name" + "column name TYPE" lines, "BULK_INSERT name" + file / fieldterminator /
 * firstrow lines).  Returns a malloc'ed string (rsq_free) or NULL with rsq_last_error set. */
char* rsq_sql_describe(rsq_ctx* ctx, const char* sql, int32_t what);

/* ---- statement loop: executeStatement (src/execute.h:508-545) over the engine ----------------
 * A database handle keeps what the reference's `Database` keeps (src/dbdata.h: relations by name): schemas from CREATE TABLE
 * (executeCreateTable, execute.h:263-281: "Table x already exists."), device-resident tables from BULK INSERT
 * (executeBulkInsert, execute.h:332-388: "Table x does not exist.", field terminator = first character of
 * `fieldterminator`, default ','), and runs SELECT statements through rsq_sql_compile + rsq_query_execute.
 * rsq_db_execute: `result` may be NULL; for a SELECT it receives a view of the result relation that stays valid until the
 * next statement on the same handle.  *kind receives 1 SELECT, 2 CREATE TABLE, 3 BULK INSERT, 4 CONTROL (may be NULL).
 * A second BULK INSERT into a table appends, as the reference's does.
 * rsq_db_adopt_table hands an existing table (rsq_table_create / _generate / ...) to the database, which then owns it.
 * Destroy a database before the context it was created on (its tables live in that context's device memory). */
typedef struct rsq_db rsq_db;
int  rsq_db_create(rsq_ctx* ctx, rsq_db** out);
int  rsq_db_execute(rsq_db* db, const char* sql, int32_t* kind, rsq_result_view* result);
/* Control statements (processControl, execute.h:454-474; *kind receives 4): `name=value` or the bare name (prints the value)
 * for showplan, tofile, threads, showperf, showasm, showfln, optimize, emitmc — spaces are ignored and, as in the reference,
 * the name may stand anywhere in the line — and `tables`.  Effects on later SELECTs: showplan puts the operator tree,
 * showperf the `compile:` / `execute:` lines of showReport (JitContextFlounder.h:132-150) plus the device figures, showasm the
 * generated HIP source, showfln the pipeline description into the message; tofile=true writes the result to "qres.tbl"
 * (serializeRelation format, execute.h:203-210, 243-245; written where rsq_ctx_set_result_text says, the host by default - the bytes
 * are the same, rsq_db_result_text_report tells which path wrote them); threads / optimize / emitmc are stored and reported only.
 * rsq_db_message: what the reference's printQueryResult prints for the last statement in front of the relation
 * (execute.h:173-200): the control statement's answer, "Created table x", "Inserted n tuples", or plan + report. */
const char* rsq_db_message(const rsq_db* db);
int  rsq_db_adopt_table(rsq_db* db, rsq_table* table);
int  rsq_db_report(const rsq_db* db, rsq_report* out);          /* of the last SELECT */
int  rsq_db_load_report(const rsq_db* db, rsq_tbl_load_report* out);      /* of the last BULK INSERT (out->struct_size set by the caller) */
int  rsq_db_result_text_report(const rsq_db* db, rsq_result_text_report* out);      /* of the last SELECT that `tofile` wrote (likewise) */
int  rsq_db_order_limit_report(const rsq_db* db, rsq_order_limit_report* out);      /* of the last SELECT (likewise) */
int  rsq_db_result_pack_report(const rsq_db* db, rsq_result_pack_report* out);      /* of the last SELECT (likewise) */
int  rsq_db_order_sort_report(const rsq_db* db, rsq_order_sort_report* out);        /* of the last SELECT (likewise) */
void rsq_db_destroy(rsq_db* db);

/* ---- one host process, N GPUs ------------------------------------------------------------------
 * JitContextFlounder::execute() fans ONE compiled function out to config.numThreads workers that pull morsels from a shared
 * iterator and joins them (reference src/JitContextFlounder.h:459-487).  The multi-GPU form of that call: a host process
 * (ReSQL's executeSelectPlan, src/execute.h:213-247, unchanged in shape) holds one handle over N GPUs; the morsels are
 * row-range shards of the scanned table, one per GPU and resident in its HBM; rsq_multi_query_execute runs the same compiled
 * pipelines on every GPU and merges the partial aggregate tables with ONE exchange step — an RCCL reduce over xGMI to the
 * root GPU (ncclReduce per [min | max | sum] segment, all segments and GPUs in one ncclGroup; communicators from
 * ncclCommInitAll; librccl is dlopen'ed by rsq_multi_create) — then finalises on the root.  Integer min / max / sum:
 * the result is bit-identical to the single-GPU one.
 *
 * Plans that do not end in a dense partial table (joins with many groups, hash aggregation, materialisation) run their
 * pipelines on every shard concurrently (every shard holds the full build-side tables) and merge on the host:
 * the GENERAL merge reads all shards' group rows (or materialised rows, in shard = scan order) back, re-aggregates groups that
 * occur in several shards by key (sum / min / max per accumulator, the smallest first row — the reference has ONE hash table
 * all its workers reach, src/operators/aggregation.h:240-295) and runs ONE tail (AVG, projection, emission order, ORDER BY,
 * LIMIT) over them: the result is the single-GPU result whatever the sharding.  Rows are numbered over the whole table for
 * that: shard tables carry their first row's number (rsq_table_generate's row0, rsq_table_set_first_row).  When the column
 * statistics prove that a group-by attribute has disjoint value ranges on the shards (the caller sharded on a boundary of
 * that key, rsq_multi_table_generate_on_key) and the plan ends in ORDER BY ... LIMIT k, every shard runs its own tail and only
 * its k leading rows are merged by the sort keys.
 *
 * devices may list a GPU more than once (shards that share a GPU: how a one-GPU box runs N shards); RCCL cannot hold a device
 * twice, so such handles — and any handle created with RSQ_MERGE_PEER_COPY — move the partial tables with peer copies to
 * the root and reduce them with the engine's merge kernel.
 *
 * Nested-loops joins (base->engine_flags has RSQ_ENGINE_NESTED_LOOPS; without it rsq_multi_query_compile refuses them,
 * RSQ_ERR_UNSUPPORTED): the plan holds one top-level RSQ_OP_NESTEDLOOPSJOIN on its last pipeline, and its pair space is split by the
 * OUTER side's rows; every shard pairs its outer rows with the WHOLE inner side in the reference's inner order, so pair ordinals
 * (outer row x inner rows + inner position, rows numbered over the whole table) and the merged result are the one-context ones.
 *   - outer table (the one the join's pipeline scans): sharded - each shard scans its own rows; replicated (equal row0, row count and
 *     statistics on every shard) - each shard scans the slice rsq_multi_shard_rows(n, N, i) of its copy.
 *   - inner side (child[0], run as a query of its own): all its tables replicated - computed on every shard; exactly one table sharded,
 *     and it is the source of the inner side's materialising pipeline - every shard computes its part and the parts are all-gathered
 *     in shard order into every shard with peer copies (its shards must hold increasing row ranges).
 *   - any other sharded table (a build side, a second inner table, one under a nested inner side): RSQ_ERR_UNSUPPORTED naming it.
 * rsq_config.nested_loops_max_pairs bounds the statement: total outer rows x total inner rows, checked after the gather and before
 * any outer pipeline runs.  The report counts the inner sides' kernels and bytes, rsq_multi_query_collective_ms includes the gather,
 * rsq_multi_query_merge_name states the split ("nested-loops: outer rows over N shards, inner side gathered (...)" / "replicated").
 * Every shard slices the inner range of its own launch (nested_loops_inner_slices of the base config, its own outer rows, the whole
 * inner side's rows).
 *
 * Derived aggregations (an aggregation below a selection, a join or another aggregation; base->engine_flags has RSQ_ENGINE_DERIVED_MULTI;
 * without it rsq_multi_query_compile refuses them, RSQ_ERR_UNSUPPORTED).  Every derived table is built on every shard before the plan's
 * pipelines run, innermost first, and equals the one-context table over the whole tables (rows, emission order, AVG, CHAR spelling):
 *   - local: every table its sub-query reads is replicated (a derived table below counts as replicated) - each shard computes it;
 *   - merged: exactly one of them is sharded and it is the source of the sub-query's aggregating pipeline - the shards' groups are
 *     merged on the root (on the device with peer copies where one context would take its device tail, else on the host) and the
 *     table goes to every shard;
 *   - any other sharded table under a derived aggregation, or a sharded build side of the plan: RSQ_ERR_UNSUPPORTED naming it.
 * A derived table that the plan's last pipeline scans is scanned slice by slice (rsq_multi_shard_rows of its rows); elsewhere every
 * shard holds it whole.  The other tables keep the contract above: the last pipeline's ordinary source is the caller's shard.  Plans with
 * both a nested-loops join and a derived aggregation are refused.  The report counts every shard's sub-queries, the collective time
 * includes the exchanges, and rsq_multi_query_merge_name states the split ("derived0 merged on the device over 3 shards (B bytes),
 * sliced", "derived0 local, whole"). */
enum rsq_merge_mode { RSQ_MERGE_AUTO = 0, RSQ_MERGE_RCCL = 1, RSQ_MERGE_PEER_COPY = 2 };
typedef struct rsq_multi_config {
    uint32_t struct_size;       /* sizeof(rsq_multi_config) of the header the host was compiled against (as rsq_config.struct_size) */
    int32_t n_devices;
    const rsq_config* base;     /* per-GPU context settings (NULL: the defaults); base->device is ignored.  A pointer, not a member: rsq_config
                                 * grows behind its own struct_size without moving the fields of this struct */
    const int32_t* devices;     /* HIP device ordinals, one shard each; devices[0] is the root */
    int32_t merge;              /* rsq_merge_mode; AUTO = RCCL when the devices are distinct */
    int32_t reserved0;
} rsq_multi_config;
typedef struct rsq_multi rsq_multi;
typedef struct rsq_multi_query rsq_multi_query;
int  rsq_multi_create(const rsq_multi_config* cfg, rsq_multi** out);
void rsq_multi_destroy(rsq_multi* m);                            /* after its queries and tables */
const char* rsq_multi_last_error(const rsq_multi* m);            /* m == NULL: of rsq_multi_create */
int32_t rsq_multi_devices(const rsq_multi* m);
rsq_ctx* rsq_multi_ctx(rsq_multi* m, int32_t shard);             /* the shard's context: create its tables on it */
const char* rsq_multi_merge_name(const rsq_multi* m);
/* rows [*row0, *row0 + *n_rows) of shard `shard` of n_shards: equal shards on 128-row tile boundaries, remainder to the last */
void rsq_multi_shard_rows(int64_t n_total, int32_t n_shards, int32_t shard, int64_t* row0, int64_t* n_rows);
/* rsq_table_generate over all shards: out_tables[i] = rows of shard i of an n_rows_total table, on GPU i */
int  rsq_multi_table_generate(rsq_multi* m, int32_t kind, int64_t n_rows_total, double scale_factor, int64_t param, uint64_t seed,
                              rsq_table** out_tables /* [n_devices] */);
/* The same with every shard boundary moved forward to the next change of `key_column` (an integer column the table is clustered
 * by, e.g. lineitem's l_orderkey): no key value spans two shards, which lets plans grouped by that key take the short merge
 * below.  Correctness never depends on it. */
int  rsq_multi_table_generate_on_key(rsq_multi* m, int32_t kind, int64_t n_rows_total, double scale_factor, int64_t param, uint64_t seed,
                                     const char* key_column, rsq_table** out_tables /* [n_devices] */);
/* tables[shard * n_tables + t] is table t of the plan on that shard's context */
int  rsq_multi_query_compile(rsq_multi* m, const rsq_plan_desc* plan, rsq_table* const* tables, int32_t n_tables, rsq_multi_query** out);
int  rsq_multi_query_execute(rsq_multi_query* q);                /* blocking, like JitContextFlounder::execute() */
int  rsq_multi_query_result(rsq_multi_query* q, rsq_result_view* out);
/* kernel_time_ms = the slowest shard's; shard_kernel_ms (may be NULL) receives every shard's */
int  rsq_multi_query_report(const rsq_multi_query* q, rsq_report* out, double* shard_kernel_ms /* [n_devices] */);
/* device time of the last execution's group-by merge (RCCL reduce / peer copies + merge kernel): an event pair on the root GPU's
 * stream around it, so it includes the root's wait for the slowest shard; 0 for one shard without a collective and for host merges */
double rsq_multi_query_collective_ms(const rsq_multi_query* q);
/* which merge the query takes and why (dense partial tables / ordered merge of LIMIT-ed rows / general merge), for logs and tests */
const char* rsq_multi_query_merge_name(const rsq_multi_query* q);
/* rsq_query_explain of one shard's statement (NULL: no such shard). */
const char* rsq_multi_query_explain(const rsq_multi_query* q, int32_t shard);
void rsq_multi_query_destroy(rsq_multi_query* q);

/* Sustained read-only streaming bandwidth of this GPU (grid-stride int64 sum over `bytes` of
 * resident memory): the measured roofline SURVEY.md §8(d) quotes fractions against. */
int  rsq_measure_read_bandwidth(rsq_ctx* ctx, size_t bytes, int32_t iters, double* gb_per_s);

#ifdef __cplusplus
}
#endif
#endif /* RESQL_HIP_H */

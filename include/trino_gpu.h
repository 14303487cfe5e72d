/* trino_gpu.h — C-ABI drop-in boundary for Trino's columnar operator hot path,
 * MI355X-native implementation (libtrino_gpu.so).
 *
 * Each entry point mirrors the io.trino SPI/operator interface a JNI shim would
 * bind (the reference has no native code; this is the surface LocalExecutionPlanner
 * -constructed operator factories would delegate to). Reference interfaces mirrored:
 *   - Page/Block:   core/trino-spi/src/main/java/io/trino/spi/Page.java:31,50-51
 *                   spi/block/Block.java:21-24 (ValueBlock|DictionaryBlock|RLE),
 *                   spi/block/LongArrayBlock.java:39-43 (flat values + valid bitmap),
 *                   spi/block/VariableWidthBlock.java:43-48, DictionaryBlock.java:55-58
 *   - SelectedPositions: operator/project/SelectedPositions.java:27-58
 *   - Operator:     operator/Operator.java:18-50
 *                   (needsInput()/addInput(Page)/getOutput()/finish()/isFinished())
 *   - OperatorFactory creation sites: sql/planner/LocalExecutionPlanner.java:2121
 *                   (scan+filter+project), :4080 (hash agg), :2966/:3017 (hash build),
 *                   OperatorFactories.java:24-47 (lookup join),
 *                   operator/output/PartitionedOutputOperator.java (partitioned output)
 * No torch types; plain pointers and sizes only. See INTEGRATION.md for the JNI
 * binding a Trino maintainer would add.
 */
#ifndef TRINO_GPU_H
#define TRINO_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (mirrors unchecked TrinoException at the boundary) ---- */
typedef enum {
    TG_OK = 0,
    TG_ERR_INVALID_ARG = 1,
    TG_ERR_NO_GPU = 2,        /* HIP device unavailable: the product path FAILS, no CPU fallback */
    TG_ERR_OOM = 3,
    TG_ERR_STATE = 4,         /* operator state machine violation */
    TG_ERR_HIP = 5,           /* underlying HIP error; see tg_last_error() */
    TG_ERR_UNSUPPORTED = 6
} tg_status;

const char* tg_last_error(void);
/* library version / build arch probe */
const char* tg_version(void);

/* ---- types (spi/type): the subset on the hot path ---- */
typedef enum {
    TG_BIGINT = 0,   /* i64  (LongArrayBlock)   */
    TG_INTEGER = 1,  /* i32  (IntArrayBlock)    */
    TG_SMALLINT = 2, /* i16  (ShortArrayBlock)  */
    TG_TINYINT = 3,  /* i8   (ByteArrayBlock)   */
    TG_DOUBLE = 4,   /* f64  (LongArrayBlock bits) */
    TG_DATE = 5,     /* i32 epoch days (IntArrayBlock) */
    TG_BOOLEAN = 6,  /* i8   (ByteArrayBlock)   */
    TG_VARCHAR = 7   /* VariableWidthBlock      */
} tg_type;

typedef enum { TG_BK_VALUE = 0, TG_BK_DICTIONARY = 1, TG_BK_RLE = 2 } tg_block_kind;

/* Flat column descriptor. Pointers may be HOST or DEVICE memory; `on_device`
 * says which. Host blocks are uploaded (flat memcpy of the backing arrays —
 * zero pivot) on addInput. */
typedef struct tg_block {
    int32_t type;               /* tg_type */
    int32_t kind;               /* tg_block_kind */
    int64_t position_count;
    int32_t on_device;          /* 0 = host pointers, 1 = device pointers */
    int32_t _pad;
    const void* data;           /* fixed-width values, or utf8 bytes for VARCHAR */
    const uint64_t* valid;      /* packed bitmap, bit=1 => valid (LongArrayBlock.valueIsValid); NULL => no nulls */
    const int32_t* offsets;     /* VARCHAR: N+1 offsets into data */
    const int32_t* ids;         /* DICTIONARY: position -> dictionary id */
    const struct tg_block* dictionary; /* DICTIONARY/RLE: the value block */
} tg_block;

typedef struct tg_page {
    int32_t channel_count;
    int64_t position_count;
    const tg_block* blocks;     /* array[channel_count] */
} tg_page;

/* SelectedPositions (operator/project/SelectedPositions.java:27-58) */
typedef struct tg_selected {
    int32_t is_list;            /* 0: range [offset, offset+size); 1: positions list */
    int32_t offset;
    int32_t size;
    const int32_t* positions;   /* when is_list */
} tg_selected;

/* ---- session = device context ---- */
typedef struct tg_session tg_session;
tg_status tg_session_create(int device_ordinal, tg_session** out);
void      tg_session_close(tg_session*);

/* ---- expression IR (replaces per-query bytecode gen, sql/gen/columnar/) ----
 * Postfix program over f64/i64 lanes; enough for TPC-H filter/project forms.
 * Integer columns and CONST_I64 stay in an exact int64 lane; an operation
 * with a DOUBLE on either side coerces the other to double. Integer division
 * truncates toward zero and integer `/ 0` is NULL (Trino raises; the ABI has
 * no per-row error channel), so a projection with a DIV carries a validity
 * bitmap even over NULL-free inputs. Integer overflow is undefined. AND / OR /
 * NOT / BETWEEN are Kleene logic; a filter keeps a row iff the result is
 * non-NULL and non-zero.
 * NULL handling: TG_EXPR_IS_NULL, TG_EXPR_COALESCE and TG_EXPR_CONST_NULL test,
 * replace and produce NULL; TG_EXPR_SELECT is the two-armed conditional that
 * CASE / IF / NULLIF are written with (both arms are evaluated: the IR has no
 * per-row error). Operand order of SELECT is otherwise, cond, then, so a
 * searched CASE with n WHENs is `else, cN, vN, SELECT, ..., c1, v1, SELECT`
 * at a depth of 3 plus its deepest operand, whatever n is. IF(c, a, b) is
 * `b, c, a, SELECT`; NULLIF(a, b) is `a, a, b, EQ, NULL, SELECT`.
 * Lanes: the lane (int64 or double) of every stack value depends only on the
 * program and the page's column types, never on the row: a NULL cell keeps
 * its column's lane. SELECT and COALESCE give an int64 result iff both value
 * operands are int64; otherwise an int64 operand is converted as (double)i.
 * Set membership: TG_EXPR_IN_LIST with arg0 = k is followed by k
 * TG_EXPR_IN_ITEM instructions, one BIGINT item each in imm.i64 (duplicates
 * and any order allowed; 1 <= k <= 4096). The result is NULL for a NULL
 * operand, else 1 / 0. An int64 operand compares exactly; a double operand d
 * compares as d == (double)item, so NaN gives 0. A NULL item has no encoding:
 * `x IN (1, NULL)` is `IN_LIST ... CONST_NULL OR`; NOT IN is `IN_LIST ... NOT`.
 * Validation (host side, before anything is launched; tg_expr_check below
 * runs the create-time part without a session): a program must reduce
 * to one value (else TG_ERR_INVALID_ARG) within 6 stack slots and use only
 * the opcodes 0..16 and 32..37 (else TG_ERR_UNSUPPORTED; more than 4096 items
 * in one list also); an IN_LIST with k < 1, with fewer than k IN_ITEMs after
 * it, an IN_ITEM anywhere else, and a CONST_NULL arg0 outside {0, 1} are
 * TG_ERR_INVALID_ARG. When a page arrives, every TG_EXPR_COL index must lie
 * inside its channels (TG_ERR_INVALID_ARG), and a VARCHAR channel may only be
 * named by a one-instruction identity projection (TG_ERR_UNSUPPORTED
 * otherwise). */
typedef enum {
    TG_EXPR_COL = 0,       /* push column[arg0] value */
    TG_EXPR_CONST_F64 = 1, /* push f64 constant */
    TG_EXPR_CONST_I64 = 2, /* push i64 constant */
    TG_EXPR_ADD = 3, TG_EXPR_SUB = 4, TG_EXPR_MUL = 5, TG_EXPR_DIV = 6,
    /* comparisons produce boolean (filter roots) */
    TG_EXPR_LE = 7, TG_EXPR_LT = 8, TG_EXPR_GE = 9, TG_EXPR_GT = 10,
    TG_EXPR_EQ = 11, TG_EXPR_NE = 12,
    TG_EXPR_AND = 13, TG_EXPR_OR = 14, TG_EXPR_NOT = 15,
    TG_EXPR_BETWEEN = 16,  /* value, lo, hi on stack */
    TG_EXPR_IN_I64 = 17,   /* reserved and unimplemented (as 18..31): rejected
                              with TG_ERR_UNSUPPORTED. The working form of IN
                              is TG_EXPR_IN_LIST */
    TG_EXPR_IS_NULL = 32,  /* pop a; push 1 if a is NULL else 0 (never NULL) */
    TG_EXPR_SELECT = 33,   /* otherwise, cond, then on stack; `then` if cond is
                              non-NULL and non-zero, else `otherwise` */
    TG_EXPR_COALESCE = 34, /* a, b on stack; a if a is non-NULL, else b */
    TG_EXPR_CONST_NULL = 35, /* push NULL; arg0 = 0 int64 lane, 1 double lane */
    TG_EXPR_IN_LIST = 36,  /* pop a; arg0 = k, the next k instructions are
                              TG_EXPR_IN_ITEM; push a IN (items) */
    TG_EXPR_IN_ITEM = 37   /* one BIGINT item of the preceding IN_LIST in
                              imm.i64; no stack effect */
} tg_expr_op;

typedef struct tg_expr_inst {
    int32_t op;
    int32_t arg0;
    union { double f64; int64_t i64; } imm;
} tg_expr_inst;

typedef struct tg_expr { const tg_expr_inst* insts; int32_t count; } tg_expr;

/* The create-time validation of a program, on the host alone: needs no
 * session and no GPU. Returns the status, and leaves in tg_last_error the
 * text, that tg_filter_run / tg_filter_project_create give for the program. */
tg_status tg_expr_check(const tg_expr* e);
/* The representation a compiled program gives an IN list with these items,
 * host only: 0 = one 64-bit mask (max - min < 64), 1 = a bitmap (max - min <
 * 4096), 2 = a sorted array; -1 for no items. Only a list that directly
 * follows a TG_EXPR_COL of an integer column is tested through it (the
 * conjunction kernel); everywhere else the interpreter searches the sorted
 * items inside the program. */
int32_t tg_expr_in_form(const int64_t* items, int32_t n);

/* ---- generic operator handle (operator/Operator.java:18-50) ---- */
typedef struct tg_operator tg_operator;
int       tg_operator_needs_input(tg_operator*);
tg_status tg_operator_add_input(tg_operator*, const tg_page*);
/* getOutput: fills out_page with DEVICE-resident blocks owned by the operator
 * until the next call; returns TG_OK with out_page->position_count==0 and
 * channel_count==0 when no output is ready. *finished set when drained. */
tg_status tg_operator_get_output(tg_operator*, tg_page* out_page, int* finished);
tg_status tg_operator_finish(tg_operator*);
void      tg_operator_close(tg_operator*);

/* ---- FilterAndProject (ScanFilterAndProjectOperator.java:66 /
 *      PageProcessor.java:102-138; filter = ColumnarFilter.java:42-52) ---- */
tg_status tg_filter_project_create(tg_session*,
    const tg_expr* filter,            /* NULL = select all */
    const tg_expr* projections,       /* array[n_proj] */
    const int32_t* proj_out_types,    /* tg_type per projection */
    int32_t n_proj,
    tg_operator** out);

/* Standalone columnar filter: predicate -> selection vector
 * (ColumnarFilter.filterPositionsRange/List). Synchronous helper used by tests.
 * A range selection must lie inside the page (TG_ERR_INVALID_ARG); a list's
 * entries are echoed in list order. A DICTIONARY / RLE block is NULL at a row
 * when its own bitmap or its dictionary's bitmap says so. */
tg_status tg_filter_run(tg_session*, const tg_expr* filter, const tg_page* page,
                        const tg_selected* input_sel,
                        int32_t* out_positions, int32_t* out_count);

/* ---- HashAggregation (HashAggregationOperator; builder
 *      InMemoryHashAggregationBuilder.java:140-158) ---- */
typedef enum { TG_STEP_PARTIAL = 0, TG_STEP_FINAL = 1, TG_STEP_SINGLE = 2 } tg_agg_step;
typedef enum {
    TG_AGG_COUNT_STAR = 0,  /* CountAggregation */
    TG_AGG_COUNT_COL  = 1,
    TG_AGG_SUM_F64    = 2,  /* DoubleSumAggregation.java:37-45 */
    TG_AGG_SUM_I64    = 3,  /* BigintSumAggregation */
    TG_AGG_AVG_F64    = 4,  /* DoubleAverageAggregations.java:38-63 (state: count,sum) */
    /* exact fixed-point double sum: the caller asserts value*2^scale_pow is
     * an integer for every input (true for TPC-H money/discount columns,
     * DESIGN.md §4) and |sum*2^scale_pow| < 2^127. State is a 128-bit
     * integer accumulated with carry-propagating 64-bit atomics:
     * order-INDEPENDENT, so the result is deterministic and correctly
     * rounded — stronger than the reference's DoubleSumAggregation, equal
     * to its decimal SUM semantics. */
    TG_AGG_SUM_F64_EXACT = 5,
    /* min/max over BIGINT (MinAggregationFunction/MaxAggregationFunction for
     * BIGINT inputs): null-skipping; state = sign-bit-biased u64 extremes */
    TG_AGG_MIN_I64 = 6,
    TG_AGG_MAX_I64 = 7
} tg_agg_fn;
typedef struct tg_agg_spec {
    int32_t fn;
    int32_t input_channel;
    int32_t scale_pow;      /* TG_AGG_SUM_F64_EXACT only; else 0 */
    /* masked aggregation (AggregationMask analog, predicate form): the row
     * contributes to THIS aggregate only when col[mask_gt_a] > col[mask_gt_b]
     * (filter clause lowered into the accumulator; -1 = unmasked). Lets one
     * pass compute filtered and unfiltered aggregates side by side. A NULL
     * in either mask cell fails the gate. Mask channels are integer/date
     * typed: a DOUBLE or VARCHAR mask channel makes add_input return
     * TG_ERR_UNSUPPORTED (channel types arrive with the first page). */
    int32_t mask_gt_a;
    int32_t mask_gt_b;
    int32_t _pad;
} tg_agg_spec;

/* StreamingAggregationOperator analog: input grouped (clustered) by a
 * single non-null BIGINT key channel — no hash table; group ids are run
 * indexes (first-occurrence row order), page-spanning runs continue. */
tg_status tg_streaming_aggregation_create(tg_session*, int32_t key_channel,
    const tg_agg_spec* aggs, int32_t n_aggs, int32_t step, tg_operator** out);
tg_status tg_hash_aggregation_create(tg_session*,
    const int32_t* group_channels, int32_t n_group_channels,
    const int32_t* group_types,               /* tg_type per group channel */
    const tg_agg_spec* aggs, int32_t n_aggs,
    int32_t step,                              /* tg_agg_step */
    tg_operator** out);

/* ---- Hash join (HashBuilderOperator nonspilling + LookupJoinOperator) ---- */
typedef struct tg_join_bridge tg_join_bridge;   /* JoinBridgeManager analog */
tg_status tg_join_bridge_create(tg_session*, tg_join_bridge** out);
void      tg_join_bridge_close(tg_join_bridge*);

tg_status tg_hash_builder_create(tg_session*, tg_join_bridge*,
    const int32_t* build_types, int32_t n_build_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* output_channels, int32_t n_output_channels,
    tg_operator** out);

/* join_type: 0 = inner, 1 = probe-outer (LEFT: unmatched probe rows emit
 * one row with a NULL build side — LookupJoinOperators probe-outer; every
 * build output column, VARCHAR included, carries a cleared validity bit).
 * Output order: probe rows ascending, the build rows matching one probe row
 * descending by global build row (reverse insertion).
 * Key equality is SQL `=`: a key with a NULL component never matches;
 * DOUBLE components compare with IEEE == (-0.0 matches 0.0, NaN matches
 * nothing, itself included) — unlike grouping, where all NaNs are one key.
 * The probe's key channels must equal the build's in count and, position by
 * position, in type: add_input rejects anything else with
 * TG_ERR_INVALID_ARG (channel types arrive with the first page).
 * join_type 2 = build-outer (RIGHT) and 3 = FULL (LookupJoinOperators
 * buildOuter): the operator emits exactly what join_type 0, respectively 1,
 * emits on the same inputs, and records on the bridge which build rows it
 * matched; tg_lookup_outer_create then emits the build rows nobody matched.
 * Such a recording operator is counted on the bridge from its creation until
 * its tg_operator_finish or tg_operator_close, so the bridge must outlive
 * it. Any other join_type is rejected with TG_ERR_INVALID_ARG. */
tg_status tg_lookup_join_create_ex(tg_session*, tg_join_bridge*,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    int32_t join_type, tg_operator** out);
/* tg_lookup_join_create_ex with a residual filter on the join condition
 * (JoinFilterFunction: `ON a.k = b.k AND <filter>`; LookupJoinOperator tests
 * it on every position of the link chain before a pair counts as a match).
 * filter == NULL is exactly tg_lookup_join_create_ex.
 * Column addressing: `filter` is a program of the expression IR above (same
 * opcodes, 6 stack slots, Kleene logic). TG_EXPR_COL index c names probe page
 * channel c when c < n_probe_channels, and build channel c - n_probe_channels
 * otherwise. Build channels are the channels given to tg_hash_builder_create,
 * all of them, not only the build output channels; probe channels need not be
 * probe output channels either.
 * Match rule: a candidate pair (probe row i, build row r) with equal keys is
 * a match iff the filter, evaluated on the cells of i and r, is non-NULL and
 * non-zero (the filter operator's keep rule). The output is the unfiltered
 * inner output with the failing pairs removed and nothing else moved: probe
 * rows ascending, the build rows of one probe row in the unfiltered order.
 * join_type 1 / 3: a probe row with no surviving pair emits one NULL-build
 * row at its place in probe order, whether its key is NULL, has no equal
 * build key, or had candidates that all failed the filter.
 * join_type 2 / 3: only surviving pairs are recorded on the bridge, so a
 * build row whose candidates all failed is emitted by tg_lookup_outer_create,
 * which is unchanged. Operators with different filters may share a bridge:
 * the visited set is the union of their surviving pairs.
 * Validation, before anything is launched. At create: the program checks of
 * tg_filter_project_create, where a program that does not reduce to one value
 * or needs more than 6 stack slots is TG_ERR_INVALID_ARG and an opcode
 * outside 0..16 is TG_ERR_UNSUPPORTED; join_type as tg_lookup_join_create_ex.
 * At add_input (page types and the built bridge are known then): a column
 * index outside n_probe_channels + build channels, or a probe index outside
 * the page, is TG_ERR_INVALID_ARG; a VARCHAR channel named by the filter is
 * TG_ERR_UNSUPPORTED. More than INT32_MAX candidate pairs (equal-key pairs
 * before the filter) or output rows for one page is TG_ERR_UNSUPPORTED on
 * this path, never a silent cast. */
tg_status tg_lookup_join_create_filtered(tg_session*, tg_join_bridge*,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    int32_t join_type,            /* 0..3 as tg_lookup_join_create_ex */
    const tg_expr* filter,        /* NULL: exactly tg_lookup_join_create_ex */
    tg_operator** out);
/* Lookup-outer operator (operator/join/LookupOuterOperator.java): the source
 * operator that completes a RIGHT or FULL join. It emits one row for every
 * build row that no probe row matched, build rows whose key has a NULL or a
 * NaN component included (they can never match). Channels are the lookup
 * join's: first n_probe_output columns of the given types in which every
 * cell is NULL (cleared validity bit, zero length for VARCHAR), then the
 * bridge's build output channels gathered from the build row. Rows come in
 * ascending global build row order in ONE page; when every build row was
 * matched, or the build is empty, no page is produced and `finished` is set.
 * The visited set is the union over all recording (join_type 2 or 3) lookup
 * joins that share the bridge; a bridge nobody probed emits every build row.
 * tg_operator_get_output returns TG_ERR_STATE while the bridge is not built,
 * while a recording lookup join on it is neither finished nor closed, or
 * once a join_type 0 or 1 lookup join has probed it (its matches were not
 * recorded), and TG_ERR_UNSUPPORTED on a set-builder bridge; all of this is
 * checked before anything is launched. tg_operator_add_input returns
 * TG_ERR_STATE and needs_input is 0. The bridge must outlive the operator. */
tg_status tg_lookup_outer_create(tg_session*, tg_join_bridge*,
    const int32_t* probe_output_types, int32_t n_probe_output,
    tg_operator** out);
tg_status tg_lookup_join_create(tg_session*, tg_join_bridge*,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    tg_operator** out);

/* ---- Partitioned output (PagePartitioner.java:134-330) ----
 * Computes per-row partitions with the canonical row hash
 * (InterpretedHashGenerator.java:57-110, combine 31*h, bigint xxmix) and
 * splits the page into per-partition pages. Transport (RCCL all-to-all)
 * happens above this ABI in the rank runner. */
tg_status tg_page_partitioner_create(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition_channels,
    int32_t partition_count,
    tg_operator** out);
/* after add_input, fetch partition p's accumulated page */
tg_status tg_page_partitioner_get_partition(tg_operator*, int32_t partition,
                                            tg_page* out_page);

/* ---- synchronous row-hash helper (tests/parity): canonical row hash ---- */
tg_status tg_hash_rows(tg_session*, const tg_page* page,
                       const int32_t* channels, int32_t n_channels,
                       uint64_t* out_hashes /* host, length position_count */);

/* ---- TPC-H device generator (bench inputs; restates io.trino.tpch v1.4
 *      column streams — plugin/trino-tpch TpchRecordSet.java call sites) ---- */
typedef struct tg_tpch_lineitem_cols {
    /* all DEVICE pointers, length row_count */
    int64_t row_count;
    int64_t* orderkey;      /* may be NULL if not requested */
    int32_t* shipdate;      /* epoch days */
    double*  quantity;
    double*  extendedprice;
    double*  discount;
    double*  tax;
    uint8_t* returnflag;    /* dictionary id: 0=A 1=N 2=R */
    uint8_t* linestatus;    /* dictionary id: 0=F 1=O */
    int32_t* commitdate;    /* optional (flags bit 1) */
    int32_t* receiptdate;   /* optional (flags bit 1) */
    int64_t* partkey;       /* optional (flags bit 2) */
    uint8_t* shipmode;      /* optional (flags bit 3): dictionary id 0..6 =
                               REG AIR,AIR,RAIL,TRUCK,MAIL,FOB,SHIP */
    int64_t* tp_cents;      /* optional (flags bit 4): this line's
                               o_totalprice contribution in cents (dbgen
                               mk_order truncation; sums to o_totalprice) */
    int64_t* suppkey;       /* optional (flags bit 5): partsupp-bridge
                               l_suppkey (canonical-row verified) */
    uint8_t* shipinstruct;  /* optional (flags bit 6): dictionary id 0..3 =
                               DELIVER IN PERSON,COLLECT COD,TAKE BACK
                               RETURN,NONE (pinned) */
    /* Exact integer forms of the four numeric columns. All
     * four are set or none is: tg_tpch_lineitem_alloc fills them when the
     * memory is there, a struct built by hand leaves them NULL. Where they
     * are set, the stated equality holds bit for bit for every row, and
     * neither they nor their f64 columns are written after generation.
     * tg_q1_run reads these 7 B/row instead of the 32 B/row of f64. */
    uint8_t* quantity_u8;          /* (double)x         == quantity[i]      */
    int32_t* extendedprice_cents;  /* (double)x / 100.0 == extendedprice[i] */
    uint8_t* discount_pct;         /* (double)x / 100.0 == discount[i]      */
    uint8_t* tax_pct;              /* (double)x / 100.0 == tax[i]           */
} tg_tpch_lineitem_cols;

/* Generate lineitem rows for orders [order_start, order_start+order_count)
 * (1-based dense order index, part of 1,500,000×SF orders). Buffers must hold
 * the actual row count (tg_tpch_lineitem_rows); row_count is set on return. */
tg_status tg_tpch_gen_lineitem(tg_session*, double scale_factor,
    int64_t order_start, int64_t order_count,
    tg_tpch_lineitem_cols* cols /* in: buffers, out: row_count */);
tg_status tg_tpch_lineitem_rows(tg_session*, double scale_factor,
    int64_t order_start, int64_t order_count, int64_t* row_count_out,
    int64_t** dev_offsets_out /* optional; hipFree */);
/* allocate device buffers of the exact size and generate (bench/tests);
 * flags: bit0 = orderkey, bit1 = commitdate+receiptdate, bit2 = partkey */
tg_status tg_tpch_lineitem_alloc(tg_session*, double scale_factor,
    int64_t order_start, int64_t order_count, int flags,
    tg_tpch_lineitem_cols* out);
tg_status tg_tpch_lineitem_free(tg_session*, tg_tpch_lineitem_cols*);
tg_status tg_tpch_gen_orders(tg_session*, double scale_factor,
    int64_t order_start, int64_t order_count,
    int64_t* dev_orderkey, int64_t* dev_custkey, int32_t* dev_orderdate,
    uint8_t* dev_priority /* nullable; ids 0..4 = 1-URGENT..5-LOW */);
tg_status tg_tpch_gen_customer(tg_session*, double scale_factor,
    int64_t cust_start, int64_t cust_count,
    int64_t* dev_custkey, uint8_t* dev_mktsegment,
    uint8_t* dev_nationkey /* 0..24 or NULL */,
    int64_t* dev_acctbal_cents /* c_acctbal*100 or NULL */);
tg_status tg_tpch_gen_supplier(tg_session*, double scale_factor,
    int64_t supp_start, int64_t supp_count,
    int64_t* dev_suppkey, uint8_t* dev_nationkey /* 0..24 */);
tg_status tg_tpch_gen_part(tg_session*, double scale_factor,
    int64_t part_start, int64_t part_count,
    int64_t* dev_partkey, int16_t* dev_type_id /* 0..149 (SMALLINT: 150 ids
    overflow signed TINYINT); PROMO = >=125 */);

/* round 2: extended tables (streams pinned in oracle/tpch_text.h against
 * the reference's own sf0.01 dataset + SF1 answer fixtures).
 * part2: type 0..149, brand 11..55, container 0..39, name_ids = 5 color
 * ids/row (dists.dss colors, alphabetical). partsupp: 4 rows per part in
 * dbgen bridge order. orders3 adds derived o_orderstatus (0=F 1=O 2=P),
 * o_totalprice cents and o_comment pool slices. */
tg_status tg_tpch_gen_part2(tg_session*, double scale_factor,
    int64_t part_start, int64_t part_count, int64_t* d_partkey,
    int16_t* d_type, uint8_t* d_brand, int32_t* d_size, uint8_t* d_container,
    uint8_t* d_name_ids, int64_t* d_retail_cents);
tg_status tg_tpch_gen_partsupp(tg_session*, double scale_factor,
    int64_t part_start, int64_t part_count, int64_t* d_partkey,
    int64_t* d_suppkey, int32_t* d_availqty, int64_t* d_supplycost_cents);
tg_status tg_tpch_gen_supplier2(tg_session*, double scale_factor,
    int64_t supp_start, int64_t supp_count, int64_t* d_suppkey,
    uint8_t* d_nationkey, int64_t* d_acctbal_cents);
tg_status tg_tpch_gen_orders3(tg_session*, double scale_factor,
    int64_t order_start, int64_t order_count, int64_t* d_orderkey,
    int64_t* d_custkey, int32_t* d_orderdate, uint8_t* d_priority,
    uint8_t* d_orderstatus, int64_t* d_totalprice_cents,
    int64_t* d_cmnt_off, int32_t* d_cmnt_len);
/* 300 MiB dbgen text pool, device-resident (built host-side, cached) */
tg_status tg_tpch_pool(tg_session*, const uint8_t** d_pool);
/* LIKE over pool slices / var-width columns -> d_flags[i] = 0 or 1
 * (LikeFunctions semantics, '%' the only wildcard, bytes not characters, no
 * escape). Forms: 'abc' exact (text == "abc"); 'abc%' prefix; '%abc' suffix;
 * '%abc%' floating; 'a%b%c' pins the first segment to the start and the last
 * to the end, the segments between are found leftmost and never overlap
 * ('ab%ab' needs four bytes). '' matches only the empty text; '%' and '%%'
 * match every text. Limits: at most 4 literal segments and 63 pattern bytes;
 * any '_' is rejected; all three are TG_ERR_UNSUPPORTED. A null session,
 * pointer or pattern, or n < 0, is TG_ERR_INVALID_ARG. Every rejection
 * happens before anything is launched, so d_flags is untouched; n == 0
 * returns TG_OK and writes nothing. The flags carry no NULL: a NULL row's
 * flag is whatever its bytes give, and the caller masks it with the
 * column's validity. tg_pool_like_flags picks its path by TG_LIKE_IDX, read
 * on every call (0 byte scan, 1 occurrence index for floating patterns,
 * 2 offset-sorted scan; unset: 2 from 2^20 rows, else 0). */
tg_status tg_pool_like_flags(tg_session*, const int64_t* d_offs,
    const int32_t* d_lens, int64_t n, const char* pattern, uint8_t* d_flags);
tg_status tg_varchar_like_flags(tg_session*, const uint8_t* d_bytes,
    const int32_t* d_offsets, int64_t n, const char* pattern, uint8_t* d_flags);
/* host-only hook for tests and host drivers (no session, no GPU): *out =
 * (bytes[0, len) LIKE pattern) through the same matcher the kernels run
 * (csrc/like_match.h). Same rejections as above; len == 0 may pass NULL. */
tg_status tg_like_match_host(const char* pattern, const uint8_t* bytes,
    int32_t len, int32_t* out);
/* s_comment var-width column incl. the BBB "Customer ...Complaints/
 * Recommends" overlay (10 rows per 10,000 suppliers) */
tg_status tg_tpch_gen_supplier_comments(tg_session*, double scale_factor,
    int64_t supp_start, int64_t supp_count, int32_t** d_offsets_out,
    uint8_t** d_bytes_out);
/* host-side string materialization for final output assembly (few rows) */
tg_status tg_tpch_supplier_strings(double sf, const int64_t* keys, int32_t n,
    int32_t stride, char* name, char* address, char* phone, char* comment,
    int64_t* acctbal_cents, int32_t* nationkey);
tg_status tg_tpch_customer_strings(double sf, const int64_t* keys, int32_t n,
    int32_t stride, char* name, char* address, char* phone, char* comment,
    int64_t* acctbal_cents, int32_t* nationkey);
tg_status tg_tpch_part_strings(double sf, const int64_t* keys, int32_t n,
    int32_t stride, char* name, char* mfgr, char* brand, char* type,
    char* container);
tg_status tg_tpch_nation_name(int32_t nationkey, char out[32]);
int32_t tg_tpch_nation_region(int32_t nationkey);
/* p_name predicate flags over the 5 color ids per part (green=33 forest=28) */
tg_status tg_tpch_part_name_flag(tg_session*, const uint8_t* d_name_ids,
    int64_t n, int32_t color_id, int32_t first_only, uint8_t* d_flags);
/* fused dynamic filter (sql/gen/columnar/DynamicPageFilter.java +
 * operator/DynamicFilterSourceOperator.java analog): request a dense-range
 * membership bitmap over the build keys BEFORE the build finishes, then
 * create the probe-side scan with the bridge attached — the membership test
 * runs inside the scan's filter kernel after the static predicate. Best
 * effort like the reference: generic/multi-channel keys or ranges beyond
 * 2^33 skip the bitmap and the scan runs the static filter alone.
 * df_key_channel must be an integer-typed channel of the probe page (BIGINT,
 * INTEGER, DATE, SMALLINT, TINYINT or BOOLEAN, each read at its own width): a
 * DOUBLE or VARCHAR channel makes add_input return TG_ERR_UNSUPPORTED, an
 * index outside the page TG_ERR_INVALID_ARG. A NULL key fails the filter. */
tg_status tg_join_bridge_request_bitmap(tg_join_bridge*);
tg_status tg_filter_project_create_df(tg_session*, const tg_expr* filter,
    const tg_expr* projections, const int32_t* proj_out_types, int32_t n_proj,
    tg_join_bridge* df_bridge, int32_t df_key_channel, tg_operator** out);

/* ---- native Parquet reader (csrc/parquet.cpp; mirrors
 * lib/trino-parquet/reader/ParquetReader.java surface) ---- */
typedef struct tg_parquet_file tg_parquet_file;
tg_status tg_parquet_open(tg_session*, const char* path, tg_parquet_file**);
void tg_parquet_close(tg_parquet_file*);
int64_t tg_parquet_num_rows(tg_parquet_file*);
int32_t tg_parquet_num_columns(tg_parquet_file*);
const char* tg_parquet_column_name(tg_parquet_file*, int32_t);
int32_t tg_parquet_physical_type(tg_parquet_file*, int32_t);
tg_status tg_parquet_read_column(tg_session*, tg_parquet_file*, int32_t col,
    void* out_values, uint64_t* out_valid, int32_t* out_ids,
    uint8_t* out_dict_bytes, int64_t dict_bytes_cap,
    int32_t* out_dict_offsets, int32_t* out_dict_count);
/* multi-column parallel decode (columns x row groups nested) */
tg_status tg_parquet_read_columns(tg_session*, tg_parquet_file*,
    const int32_t* cols, int32_t n_cols, void** out_values,
    uint64_t** out_valid, int32_t** out_ids, uint8_t** out_dict_bytes,
    const int64_t* dict_caps, int32_t** out_dict_offsets,
    int32_t** out_dict_counts);

tg_status tg_copy_dtod(tg_session*, void* dst_dev, const void* src_dev,
                       int64_t bytes);

/* adaptive partial aggregation (operator/aggregation/partial/
 * PartialAggregationController.java:34-100 analog): one controller is
 * shared across the PARTIAL-step hash aggregations of a plan node. After
 * >= 1.5x max_partial_bytes of input has been sampled, if the ratio of
 * unique output rows to input rows exceeds the threshold (reference
 * session default 0.8 — adaptive_partial_aggregation_unique_rows_ratio_
 * threshold), partial aggregation flips to pass-through: pages are
 * re-shaped into the partial-state channel layout with no hash-table work
 * and the FINAL stage does the grouping. Re-enabled after 200x more bytes
 * (same constants as the reference). on_flush is exposed so host drivers
 * (and CPU tests) can feed flush statistics directly. Restrictions:
 * fixed-width group keys, unmasked aggregates. */
typedef struct tg_pa_controller tg_pa_controller;
tg_status tg_pa_controller_create(int64_t max_partial_bytes,
    double unique_rows_ratio_threshold, tg_pa_controller** out);
void tg_pa_controller_close(tg_pa_controller*);
int32_t tg_pa_controller_disabled(tg_pa_controller*);
tg_status tg_pa_controller_on_flush(tg_pa_controller*, int64_t bytes,
    int64_t rows, int64_t unique_rows, int32_t have_unique);
tg_status tg_hash_aggregation_set_controller(tg_operator*, tg_pa_controller*);

/* MarkDistinctOperator analog: appends a BOOLEAN channel marking each
 * row's first occurrence over the key channels (streaming pass-through:
 * every add_input stages its page, input channels unchanged with their
 * validity, then the flag channel, which has no bitmap). 0..7 key channels
 * of any type. NULL is a key value in every position ((NULL,1), (NULL,2),
 * (NULL,NULL) are three keys), every NaN is one key, -0.0 is 0.0, VARCHAR
 * compares by bytes and '' is not NULL. Zero key channels: only the first
 * row of the whole input is flagged. Zero-row pages are accepted anywhere,
 * VARCHAR keys included, and come out as zero-row pages. */
tg_status tg_mark_distinct_create(tg_session*, const int32_t* key_channels,
    int32_t n_key_channels, const int32_t* key_types, tg_operator**);

/* dense-range single-BIGINT-key aggregation (direct array state, one
 * atomic per row — or an atomic pair for the 128-bit exact sum; groups
 * emit in key order). For COUNT/SUM_I64/SUM_F64_EXACT over keys with
 * known dense statistics (generated custkeys/suppkeys).
 * Contract: every non-NULL key in [key_min, key_max] that occurs in the
 * input is emitted as a group, also when its aggregate is 0 (a SUM that
 * cancels, a COUNT_COL over only NULL values). Rows whose key is NULL or
 * outside [key_min, key_max] are DROPPED silently — unlike a hash
 * aggregation, which would group them; the caller guarantees the range. */
tg_status tg_dense_aggregation_create(tg_session*, int32_t key_channel,
    int64_t key_min, int64_t key_max, const tg_agg_spec* agg, tg_operator**);

/* sort-based DISTINCT of a non-negative BIGINT device column (radix sort +
 * unique compaction; `bits` = key width to sort). For near-all-unique
 * dedups (count(DISTINCT ...)) where hash aggregation pays random keystore
 * probes per row. d_out sized n; *out_n gets the distinct count and d_out
 * the distinct keys ascending. Every key must lie in [0, 2^bits) (bits = 64:
 * [0, 2^63)); nothing checks it, a check would cost a pass over the
 * column. Only the low `bits` bits order the sort, so with a wider key the
 * output may be unsorted and may repeat a key, but it loses and invents
 * none. n = 0 gives 0. A null pointer, n < 0 or bits outside 1..64 is
 * TG_ERR_INVALID_ARG before anything is launched. */
tg_status tg_dedup_i64(tg_session*, const int64_t* d_in, int64_t n,
    int32_t bits, int64_t* d_out, int64_t* out_n);

/* stream timer (HIP events on the session stream) for bench rooflines */
tg_status tg_timer_start(tg_session*);
tg_status tg_timer_stop(tg_session*, double* elapsed_ms);

/* coarse device-memory accounting (LocalMemoryContext analog): bytes ever
 * pooled and bytes currently cached; live = total - cached */
tg_status tg_session_memory(tg_session*, int64_t* total_bytes, int64_t* cached_bytes);

/* device buffer management for host pipeline drivers (pool-backed) */
tg_status tg_device_malloc(tg_session*, void** out, int64_t bytes);
tg_status tg_device_free(tg_session*, void* p);

/* ---- TopN (operator/TopNOperator.java): ORDER BY ... LIMIT ----
 * sort_desc[i]: 0 = ASC (nulls last), 1 = DESC (nulls first).
 * DOUBLE keys order numerically with -0.0 == +0.0, and every NaN (either sign
 * bit, any payload) ranks as the single largest non-NULL value (Trino's
 * ORDER BY rule): ASC ... +inf, NaN, NULL; DESC NULL, NaN, +inf ... NULL is
 * ordered apart from every value, INT64_MAX and NaN included. Order among
 * rows whose whole sort key ties is unspecified. Every output channel carries
 * its rows' validity. Channels are fixed-width: a VARCHAR channel is rejected
 * with TG_ERR_UNSUPPORTED, a sort channel outside the channels and a page
 * whose cell widths differ from `types` with TG_ERR_INVALID_ARG. */
tg_status tg_topn_create(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t limit, tg_operator** out);

/* ---- OrderBy (operator/OrderByOperator.java): ORDER BY without LIMIT, and
 * TopN over any channel types, VARCHAR included ----
 * tg_order_by_create accumulates pages and emits every row, ordered, as ONE
 * page at finish. tg_topn_create_ex is tg_topn_create with VARCHAR allowed:
 * the first `limit` rows of what tg_order_by_create emits for the same
 * arguments with every channel output.
 *
 * Ordering rules. Keys are most significant first. sort_desc[i]: 0 = ASC
 * nulls last, 1 = DESC nulls first. Fixed-width keys follow tg_topn_create's
 * rule exactly: NaN is the largest non-NULL value, -0.0 == 0.0. A VARCHAR key
 * orders by unsigned bytes, lexicographically, and a proper prefix sorts
 * first (VarcharType / Slice.compareTo):
 *     '' < '\0' < '\0\0' < 'a' < 'a\0' < 'ab' < '\x7f' < '\x80'
 * '' is a value, not NULL. Rows whose whole key ties KEEP INPUT ORDER (page
 * order, then row order), through both entry points and at every row count,
 * so outputs are reproducible bit for bit. The order always comes from the
 * device: there is no host path and no row threshold.
 *
 * Output. One page at finish; no input rows (or only zero-row pages): no
 * page, and `finished` is set. Any channel may be VARCHAR, as a key or as
 * payload. Output offsets start at 0, and a NULL VARCHAR cell has zero
 * length. A channel carries a validity bitmap exactly when some non-empty
 * input page's block had one. output_channels may select a subset, reorder,
 * or repeat a channel, and sort channels need not be output; NULL / 0 emits
 * every channel in order. For tg_topn_create_ex a limit larger than the input
 * emits everything.
 *
 * Rejected before anything is launched, TG_ERR_INVALID_ARG: a null session /
 * types / out, n_sort < 1, a sort or output channel outside the channels,
 * limit < 1, n_output < 0, a null array with a non-zero count, a type outside
 * tg_type. At add_input, TG_ERR_INVALID_ARG: a page with fewer channels than
 * declared, a fixed-width channel whose cell width differs from `types`, a
 * VARCHAR block where a fixed-width type was declared, or the reverse. At
 * add_input, TG_ERR_UNSUPPORTED: the bytes accumulated in one VARCHAR channel
 * (offsets[n] per page, the bytes the block carries) exceed INT32_MAX
 * (output offsets are int32), or the accumulated rows exceed INT32_MAX; both
 * are host-side sums, and the refused page is not kept. The operator stays usable and closable
 * after a rejected page.
 *
 * tg_topn_create, tg_window_create, tg_window_create_ex and
 * tg_topn_ranking_create are untouched: they keep rejecting VARCHAR.
 *
 * TG_VAR_COPY_LANES (a power of two, 1..64) in the environment, read at each
 * emit, overrides the lanes per row of the VARCHAR byte copy, which is
 * otherwise chosen from the mean output length. A measurement knob: the
 * result does not depend on it.
 *
 * Out of scope: VARCHAR through Window / window_ex / TopNRanking (new entry
 * points; the string image added here is what they will use), moving the
 * TPC-H queries' final host sorts onto this operator, collations other than
 * bytes, paged (multi-page) output, spilling, restricting later refinement
 * rounds of the string image to the rows that still tie. */
tg_status tg_order_by_create(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const int32_t* output_channels, int32_t n_output,   /* NULL / 0 = every channel in order */
    tg_operator** out);
tg_status tg_topn_create_ex(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t limit, tg_operator** out);

/* host-only hook for tests: *out = the chunk of bytes[0, len) in refinement
 * round `round` of the VARCHAR sort image, i.e. bytes [8 * round, 8 * round +
 * 8) big-endian, zero past len, through the very function the kernel runs
 * (csrc/var_keys.h); no session, no GPU. len == 0 may pass NULL. A null out,
 * a negative len or round: TG_ERR_INVALID_ARG. */
tg_status tg_varchar_chunk_host(const uint8_t* bytes, int32_t len, int32_t round,
    uint64_t* out);

/* ---- Window (operator/WindowOperator.java): ranking functions and running
 * aggregates OVER (PARTITION BY ... ORDER BY ...) ----
 * Pages accumulate as in TopN. At finish the operator emits ONE page: every
 * input channel, then one BIGINT channel per spec, in spec order. No input
 * rows: no page, and `finished` is set.
 *
 * Row order: by the partition channels ASC NULLS LAST (what WindowOperator
 * hands PagesIndex.sort), then by the sort channels under sort_desc with
 * TopN's rule exactly (ASC nulls last, DESC nulls first, NaN the largest
 * non-NULL value, -0.0 == 0.0). Rows whose whole partition-plus-sort key ties
 * KEEP INPUT ORDER (page order, then row order), so every output is
 * reproducible bit for bit, row_number and ROWS frames among peers included.
 * The sort always runs on the device; there is no row threshold.
 *
 * Two adjacent sorted rows share a partition iff they agree on every
 * partition channel under grouping equality: NULL is a value, all NaNs are
 * one value, -0.0 is 0.0. They are peers iff they also agree on every sort
 * channel under the same equality. n_partition == 0: one partition of
 * everything. n_sort == 0: every row of a partition is a peer of every other.
 * Both zero: no sort runs at all.
 *
 * ROW_NUMBER: 1-based position in the partition. RANK: the row_number of the
 * row's first peer. DENSE_RANK: the number of peer groups up to and including
 * the row's own. The three ignore input_channel (pass -1), require frame == 0
 * and their output has no validity bitmap.
 *
 * Aggregates run over the frame. COUNT_STAR counts rows (input_channel is
 * ignored). COUNT_COL counts the non-NULL cells of input_channel; neither
 * count has a bitmap. SUM_I64 / MIN_I64 / MAX_I64 read an integer-typed
 * channel (BIGINT, INTEGER, DATE, SMALLINT, TINYINT, BOOLEAN) widened to i64
 * and skip NULLs; their output always carries a validity bitmap, and a frame
 * that holds no non-NULL input gives NULL. SUM overflow wraps (undefined, like
 * the expression lane). FRAME_RANGE gives every row of a peer group the value
 * at the group's last row, FRAME_PARTITION the value at the partition's last
 * row.
 *
 * Rejected before anything is launched: a null session / types / out, a null
 * array with a non-zero count, n_specs outside 1..8, a partition / sort /
 * input channel outside the channels, an unknown fn or frame, a ranking spec
 * with frame != 0: TG_ERR_INVALID_ARG. Any VARCHAR channel (the payload
 * gather moves fixed-width cells, as TopN), or a DOUBLE input_channel (a
 * parallel scan reassociates the additions; an exact fixed-point running sum
 * is a later change): TG_ERR_UNSUPPORTED. At add_input, a page with fewer
 * channels than declared or with cell widths that differ from `types`:
 * TG_ERR_INVALID_ARG.
 *
 * tg_window_create takes functions 0..7 and frames 0..2 only; the functions
 * and the frame below are reached through tg_window_create_ex.
 *
 * Out of scope: IGNORE NULLS, lag / lead defaults other than NULL, RANGE /
 * GROUPS frames with offsets, DOUBLE aggregates, VARCHAR payloads, ntile /
 * percent_rank / cume_dist. A ranking cut-off (ranking <= N) is its own
 * operator: tg_topn_ranking_create below. */
typedef enum {
    TG_WIN_ROW_NUMBER = 0, TG_WIN_RANK = 1, TG_WIN_DENSE_RANK = 2,
    TG_WIN_COUNT_STAR = 3, TG_WIN_COUNT_COL = 4,
    TG_WIN_SUM_I64 = 5, TG_WIN_MIN_I64 = 6, TG_WIN_MAX_I64 = 7,
    /* tg_window_create_ex only */
    TG_WIN_LAG = 8, TG_WIN_LEAD = 9, TG_WIN_FIRST_VALUE = 10,
    TG_WIN_LAST_VALUE = 11, TG_WIN_NTH_VALUE = 12
} tg_window_fn;
typedef enum {
    TG_WIN_FRAME_RANGE = 0,     /* RANGE UNBOUNDED PRECEDING .. CURRENT ROW: the row's peers included (SQL default) */
    TG_WIN_FRAME_ROWS = 1,      /* ROWS  UNBOUNDED PRECEDING .. CURRENT ROW */
    TG_WIN_FRAME_PARTITION = 2, /* UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING */
    TG_WIN_FRAME_ROWS_BETWEEN = 3   /* ROWS BETWEEN frame_start AND frame_end; tg_window_create_ex only */
} tg_window_frame;
typedef struct tg_window_spec { int32_t fn, input_channel, frame, _pad; } tg_window_spec;

tg_status tg_window_create(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const tg_window_spec* specs, int32_t n_specs, tg_operator** out);

/* ---- Window, second entry point: bounded ROWS frames and the value
 * functions lag / lead / first_value / last_value / nth_value ----
 * Row order, partition and peer rules, page accumulation, the single output
 * page and the state machine are those of tg_window_create. A spec of the
 * functions 0..7 under the frames 0..2 (frame_start, frame_end and offset
 * zero) gives the same bits through either entry point.
 *
 * Frames. The frame of the row at sorted position i, in the partition
 * [ps, pe], is the index range [lo, hi]:
 *     FRAME_RANGE         lo = ps                        hi = the row's last peer
 *     FRAME_ROWS          lo = ps                        hi = i
 *     FRAME_PARTITION     lo = ps                        hi = pe
 *     FRAME_ROWS_BETWEEN  lo = max(ps, i + frame_start)  hi = min(pe, i + frame_end)
 * frame_start / frame_end are signed row offsets from the current row
 * (-3 = 3 PRECEDING, 0 = CURRENT ROW, 2 = 2 FOLLOWING) or the UNBOUNDED
 * values; i + offset saturates and never wraps, so frame_start = 2^62 and
 * frame_end = INT64_MAX - 1 are legal. UNBOUNDED PRECEDING gives ps,
 * UNBOUNDED FOLLOWING gives pe. lo > hi is an EMPTY frame: the offsets point
 * past the partition's edge, or frame_start > frame_end (accepted; every
 * frame is empty).
 *
 * Aggregates over FRAME_ROWS_BETWEEN: COUNT_STAR is max(0, hi - lo + 1),
 * COUNT_COL the non-NULL cells of [lo, hi]; SUM_I64 / MIN_I64 / MAX_I64 skip
 * NULLs, and an empty frame or one without a non-NULL cell gives NULL. The
 * bitmap rule is unchanged: the three value aggregates carry one, the counts
 * do not. SUM wraps and equals the wrapped sequential sum of the frame's
 * cells.
 *
 * Value functions copy a cell of input_channel, any fixed-width type, DOUBLE
 * included: NaN payloads and -0.0 come through bit for bit. The output
 * channel has the input channel's type and width and always carries a
 * validity bitmap. NULLs are respected: a NULL source cell is a NULL result.
 *     LAG         the cell at i - offset if that is >= ps, else NULL; frame 0
 *     LEAD        the cell at i + offset if that is <= pe, else NULL; frame 0
 *     FIRST_VALUE the cell at lo; an empty frame gives NULL
 *     LAST_VALUE  the cell at hi; an empty frame gives NULL
 *     NTH_VALUE   the cell at lo + offset - 1 if that is <= hi, else NULL
 * offset 0 of LAG / LEAD is the row itself; i + offset and lo + offset - 1
 * saturate. FIRST / LAST / NTH_VALUE take any of the four frames.
 *
 * Rejected before anything is launched: everything tg_window_create rejects,
 * with the same status; and with TG_ERR_INVALID_ARG: fn outside 0..12, frame
 * outside 0..3, frame_start == UNBOUNDED_FOLLOWING, frame_end ==
 * UNBOUNDED_PRECEDING, a non-zero frame_start / frame_end with a frame other
 * than ROWS_BETWEEN, a non-zero offset on a function other than LAG / LEAD /
 * NTH_VALUE, offset < 0 for LAG / LEAD, offset < 1 for NTH_VALUE, LAG / LEAD
 * or a ranking function with frame != 0, a value function's input_channel
 * outside the channels. TG_ERR_UNSUPPORTED: a DOUBLE input_channel on an
 * aggregate, VARCHAR anywhere. */
#define TG_WIN_UNBOUNDED_PRECEDING INT64_MIN
#define TG_WIN_UNBOUNDED_FOLLOWING INT64_MAX
typedef struct tg_window_spec_ex {
    int32_t fn, input_channel, frame, _pad;
    int64_t frame_start, frame_end; /* ROWS_BETWEEN only */
    int64_t offset;                 /* LAG / LEAD: rows back / forward, >= 0;
                                       NTH_VALUE: n >= 1; otherwise 0 */
} tg_window_spec_ex;                /* 40 bytes */

tg_status tg_window_create_ex(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const tg_window_spec_ex* specs, int32_t n_specs, tg_operator** out);

/* ---- TopNRanking (operator/TopNRankingOperator.java): the rows whose
 * row_number / rank / dense_rank OVER (PARTITION BY ... ORDER BY ...) is
 * <= N, i.e. `SELECT * FROM (SELECT *, fn() OVER (...) AS r FROM t) WHERE
 * r <= N` as one operator ----
 * Result: exactly the page tg_window_create emits for the same types,
 * partition channels, sort channels, sort_desc and the one ranking spec
 * (ranking_fn, -1, FRAME_RANGE), restricted to the rows whose ranking is
 * <= max_ranking_per_partition, the remaining rows in the same order.
 * emit_ranking = 1: the input channels, then the BIGINT ranking channel with
 * the same values (no validity bitmap). emit_ranking = 0: the input channels
 * only, which is the partial step: the outputs of several such operators,
 * fed to one operator with the same arguments, give the result of the whole
 * input, ties in the order the outputs were fed. One output page at finish.
 * No input rows, or only zero-row pages: no page, and `finished` is set.
 *
 * Row order, partition and peer equality, the handling of NULL / NaN / -0.0
 * and "rows whose whole partition-plus-sort key ties keep input order" are
 * the Window's (tg_window_create above), word for word.
 *
 * Row counts. ROW_NUMBER keeps at most N rows of a partition. RANK and
 * DENSE_RANK keep every peer of a kept row, so a partition can emit more
 * than N rows. n_sort == 0 makes every row of a partition a peer of every
 * other: ROW_NUMBER then keeps the partition's first N rows in input order,
 * RANK and DENSE_RANK keep everything. Every non-empty partition keeps at
 * least its first row.
 *
 * Memory. Unlike the Window, the operator does not hold its input until
 * finish: whenever the buffered rows reach max(T, 2 x the rows kept by the
 * last cut) it cuts them down to the rows that can still be emitted. T is
 * TG_TOPNR_COMPACT_ROWS (rows, >= 1) from the environment, read at create;
 * unset: 2^24. The result does not depend on T.
 *
 * Rejected before anything is launched: a null session / types / out, a null
 * array with a non-zero count, a partition / sort channel outside the
 * channels, ranking_fn outside 0..2, max_ranking_per_partition < 1,
 * emit_ranking outside 0..1: TG_ERR_INVALID_ARG. Any VARCHAR channel (the
 * payload gather moves fixed-width cells, as TopN and Window):
 * TG_ERR_UNSUPPORTED. At add_input, a page with fewer channels than declared
 * or with cell widths that differ from `types`: TG_ERR_INVALID_ARG.
 *
 * Out of scope: VARCHAR channels, percent_rank / cume_dist / ntile, a
 * hash-grouped path without a sort, spilling. */
typedef enum {
    TG_RANKING_ROW_NUMBER = 0, TG_RANKING_RANK = 1, TG_RANKING_DENSE_RANK = 2
} tg_ranking_fn;

tg_status tg_topn_ranking_create(tg_session*,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t ranking_fn,                 /* tg_ranking_fn */
    int32_t max_ranking_per_partition,  /* N >= 1 */
    int32_t emit_ranking,               /* 1: append the BIGINT ranking channel (no bitmap); 0: rows only (the partial step) */
    tg_operator** out);

/* ---- semi join (operator/HashSemiJoinOperator.java): appends a BOOLEAN
 * matched channel to the probe page. Three-valued IN: a hit is true; a NULL
 * probe key is false against a build of zero rows and NULL otherwise; a miss
 * is NULL when the build holds a NULL key, else false. Same `=` as the
 * lookup join (NaN matches nothing). One key channel: add_input rejects a
 * bridge built on several key channels with TG_ERR_UNSUPPORTED, and a probe
 * key whose type differs from the build key's with TG_ERR_INVALID_ARG. ---- */
/* SetBuilderOperator analog (ChannelSet): semi-join membership source.
 * Dense single-BIGINT key ranges build a bitmap; sparse fall back to the
 * positional index. The bridge then serves tg_semi_join_create only. */
tg_status tg_set_builder_create(tg_session*, tg_join_bridge*,
    const int32_t* build_types, int32_t n_build_channels,
    int32_t key_channel, tg_operator** out);
tg_status tg_semi_join_create(tg_session*, tg_join_bridge*,
    int32_t key_channel, tg_operator** out);

/* ---- dynamic filter source (DynamicFilterSourceOperator /
 * sql/gen/columnar/DynamicPageFilter.java analog): min/max over the build
 * side's non-null keys, valid after the builder's finish ---- */
tg_status tg_join_bridge_key_range(tg_join_bridge*, int64_t* key_min,
                                   int64_t* key_max, int64_t* key_rows);

/* test helpers */
tg_status tg_copy_dtoh(tg_session*, void* dst, const void* src, int64_t bytes);
tg_status tg_copy_htod(tg_session*, void* dst_dev, const void* src_host, int64_t bytes);

/* ---- fused TPC-H Q1 pipeline (the north-star benchmark kernel):
 * scan+filter(shipdate<=cutoff)+group(returnflag,linestatus)+7 aggregates,
 * one pass over HBM (38 B/row algorithmic). Results per (rf,ls) combo. ---- */
typedef struct tg_q1_result {
    /* indexed [rf*2+ls], rf in {A,N,R}=0,1,2; ls in {F,O}=0,1 */
    double sum_qty[6], sum_base[6], sum_disc_price[6], sum_charge[6];
    double avg_qty[6], avg_price[6], avg_disc[6];
    double sum_disc[6];
    int64_t count[6];
    double elapsed_ms;          /* kernel time, HIP events */
    /* raw integer accumulators (per combo: base,dp,ch,disc as u128 lo/hi
     * pairs then qty,cnt), for exact cross-GPU merging */
    uint64_t raw[60];
} tg_q1_result;

tg_status tg_q1_run(tg_session*, const tg_tpch_lineitem_cols* cols,
                    int32_t shipdate_cutoff, tg_q1_result* out);
/* parity mode: reference sequential accumulation order (page-sized inputs) */
tg_status tg_q1_run_naive(tg_session*, const tg_tpch_lineitem_cols* cols,
                          int32_t shipdate_cutoff, tg_q1_result* out);

#ifdef __cplusplus
}
#endif
#endif /* TRINO_GPU_H */

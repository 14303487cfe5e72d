/* expr_eval.h — the device postfix interpreter over the tg_expr IR, shared by
 * the filter / project kernels (ops_filter.hip: every column of ONE row) and
 * the join's residual filter (ops_join.hip: the columns of a probe row and a
 * build row). One interpreter, so both evaluate the same semantics; only the
 * column resolver differs.
 */
#pragma once
#include "operators.h"

struct KCol { const void* data; const uint64_t* valid; int32_t type; int32_t _pad; };

constexpr int EXPR_STACK_SLOTS = 6;   /* s0..s5 of eval_expr_cols */
constexpr int IN_LIST_MAX = 4096;     /* items of one TG_EXPR_IN_LIST */

/* Typed stack value: BIGINT/INTEGER/DATE/… stay in an exact int64 lane
 * (mirrors sql/gen/columnar/CallColumnarFilterGenerator.java:160-198 which
 * compiles the comparison at the column's Java type — long compares are
 * exact there, so they must be exact here; keys above 2^53 would silently
 * lose precision in a double lane). `f` mirrors the value for mixed-type
 * ops (Trino coerces BIGINT to DOUBLE in mixed expressions). */
struct TVal { double f; int64_t i; bool isint; bool null; };

__device__ static inline TVal load_tcol(const KCol& c, int64_t i)
{
    TVal v;
    v.null = c.valid && !((c.valid[i >> 6] >> (i & 63)) & 1);
    /* a NULL cell keeps its column's lane: SELECT / COALESCE can put a value
     * in its place, and the lane of that result must not depend on the row */
    if (v.null) { v.f = 0.0; v.i = 0; v.isint = c.type != TG_DOUBLE; return v; }
    switch (c.type) {
        case TG_BIGINT: v.i = ((const int64_t*)c.data)[i]; v.isint = true; v.f = (double)v.i; break;
        case TG_INTEGER: case TG_DATE: v.i = ((const int32_t*)c.data)[i]; v.isint = true; v.f = (double)v.i; break;
        case TG_SMALLINT: v.i = ((const int16_t*)c.data)[i]; v.isint = true; v.f = (double)v.i; break;
        case TG_TINYINT: case TG_BOOLEAN: v.i = ((const int8_t*)c.data)[i]; v.isint = true; v.f = (double)v.i; break;
        default: v.f = ((const double*)c.data)[i]; v.i = 0; v.isint = false; break;
    }
    return v;
}

__device__ static inline bool tval_truthy(const TVal& v) { return v.isint ? v.i != 0 : v.f != 0.0; }

/* column resolvers: TG_EXPR_COL index -> typed cell */
struct RowCols {            /* every column of one row */
    const KCol* cols;
    int64_t row;
    __device__ inline TVal operator()(int32_t c) const { return load_tcol(cols[c], row); }
};

struct PairCols {           /* c < n_probe: probe row cell, else build row cell */
    const KCol* pcols;
    const KCol* bcols;
    int32_t n_probe;
    int64_t prow, brow;
    __device__ inline TVal operator()(int32_t c) const
    {
        return c < n_probe ? load_tcol(pcols[c], prow) : load_tcol(bcols[c - n_probe], brow);
    }
};

/* postfix interpreter; returns a typed value. Integer ops are exact int64
 * (incl. BIGINT/BIGINT truncated division); mixed int/double coerces to
 * double. Comparisons compare in int64 iff both sides are int. AND/OR/NOT
 * follow SQL Kleene three-valued logic (io.trino.sql.ir.Logical semantics:
 * AND — false dominates null; OR — true dominates null; NOT null = null),
 * so compositions under NOT are correct; a null FILTER result rejects the
 * row at the call site (CallColumnarFilterGenerator's nullable loop).
 * SELECT / COALESCE pick one of two evaluated operands; their lane is int64
 * iff both value operands are (TVal::f mirrors every int64 value, so the
 * double lane reads .f of either). IN_LIST searches the items that follow it
 * in `prog` (sorted and de-duplicated by tg_compile_expr) and skips them. */
template <typename Cols>
__device__ static TVal eval_expr_cols(const tg_expr_inst* prog, int count, const Cols& col)
{
    TVal s0{}, s1{}, s2{}, s3{}, s4{}, s5{};
    int sp = 0;
#define PUSH(v) do { switch (sp) { \
        case 0: s0 = (v); break; case 1: s1 = (v); break; \
        case 2: s2 = (v); break; case 3: s3 = (v); break; \
        case 4: s4 = (v); break; default: s5 = (v); break; } \
        sp++; } while (0)
#define TOP (sp == 1 ? s0 : sp == 2 ? s1 : sp == 3 ? s2 : sp == 4 ? s3 \
             : sp == 5 ? s4 : s5)
#define POP(v) do { v = TOP; sp--; } while (0)
#define ARITH(expr_i, expr_f) do { TVal r; r.null = a.null | b.null; \
        r.isint = a.isint & b.isint; \
        if (r.isint) { r.i = (expr_i); r.f = (double)r.i; } \
        else { r.f = (expr_f); r.i = 0; } PUSH(r); } while (0)
#define CMP(op_) do { TVal r; r.null = a.null | b.null; r.isint = true; \
        r.i = (a.isint & b.isint) ? (a.i op_ b.i ? 1 : 0) \
                                  : (a.f op_ b.f ? 1 : 0); \
        r.f = (double)r.i; PUSH(r); } while (0)

    for (int pc = 0; pc < count; pc++) {
        tg_expr_inst in = prog[pc];
        TVal a, b, c;
        switch (in.op) {
            case TG_EXPR_COL: PUSH(col(in.arg0)); break;
            case TG_EXPR_CONST_F64: { TVal v; v.f = in.imm.f64; v.i = 0; v.isint = false; v.null = false; PUSH(v); break; }
            case TG_EXPR_CONST_I64: { TVal v; v.i = in.imm.i64; v.f = (double)v.i; v.isint = true; v.null = false; PUSH(v); break; }
            case TG_EXPR_ADD: POP(b); POP(a); ARITH(a.i + b.i, a.f + b.f); break;
            case TG_EXPR_SUB: POP(b); POP(a); ARITH(a.i - b.i, a.f - b.f); break;
            case TG_EXPR_MUL: POP(b); POP(a); ARITH(a.i * b.i, a.f * b.f); break;
            case TG_EXPR_DIV: POP(b); POP(a); {
                TVal r; r.isint = a.isint & b.isint;
                if (r.isint) {   /* BIGINT/BIGINT truncates; /0 poisons to null
                                    (the C-ABI has no per-row error channel;
                                    Trino raises DIVISION_BY_ZERO) */
                    r.null = a.null | b.null | (b.i == 0);
                    r.i = (b.i == 0) ? 0 : a.i / b.i;
                    r.f = (double)r.i;
                }
                else { r.null = a.null | b.null; r.f = a.f / b.f; r.i = 0; }
                PUSH(r); break;
            }
            case TG_EXPR_LE: POP(b); POP(a); CMP(<=); break;
            case TG_EXPR_LT: POP(b); POP(a); CMP(<); break;
            case TG_EXPR_GE: POP(b); POP(a); CMP(>=); break;
            case TG_EXPR_GT: POP(b); POP(a); CMP(>); break;
            case TG_EXPR_EQ: POP(b); POP(a); CMP(==); break;
            case TG_EXPR_NE: POP(b); POP(a); CMP(!=); break;
            case TG_EXPR_AND: { POP(b); POP(a);
                bool af = !a.null && !tval_truthy(a), bf = !b.null && !tval_truthy(b);
                TVal r; r.isint = true;
                r.null = !(af | bf) && (a.null | b.null);
                r.i = (!r.null && !af && !bf) ? 1 : 0;
                r.f = (double)r.i; PUSH(r); break;
            }
            case TG_EXPR_OR: { POP(b); POP(a);
                bool at = !a.null && tval_truthy(a), bt = !b.null && tval_truthy(b);
                TVal r; r.isint = true;
                r.null = !(at | bt) && (a.null | b.null);
                r.i = (at | bt) ? 1 : 0;
                r.f = (double)r.i; PUSH(r); break;
            }
            case TG_EXPR_NOT: { POP(a);
                TVal r; r.isint = true; r.null = a.null;
                r.i = (!a.null && !tval_truthy(a)) ? 1 : 0;
                r.f = (double)r.i; PUSH(r); break;
            }
            case TG_EXPR_BETWEEN: { POP(c); POP(b); POP(a);
                /* a >= b AND a <= c under Kleene AND, typed compares */
                bool ge, le, ge_n = a.null | b.null, le_n = a.null | c.null;
                ge = (a.isint & b.isint) ? a.i >= b.i : a.f >= b.f;
                le = (a.isint & c.isint) ? a.i <= c.i : a.f <= c.f;
                bool af = !ge_n && !ge, bf = !le_n && !le;
                TVal r; r.isint = true;
                r.null = !(af | bf) && (ge_n | le_n);
                r.i = (!r.null && !af && !bf) ? 1 : 0;
                r.f = (double)r.i; PUSH(r); break;
            }
            case TG_EXPR_IS_NULL: { POP(a);
                TVal r; r.isint = true; r.null = false;
                r.i = a.null ? 1 : 0;
                r.f = (double)r.i; PUSH(r); break;
            }
            case TG_EXPR_SELECT: { POP(c); POP(b); POP(a);   /* otherwise, cond, then */
                bool take = !b.null && tval_truthy(b);
                TVal r; r.isint = a.isint & c.isint;
                r.null = take ? c.null : a.null;
                r.f = take ? c.f : a.f;
                r.i = r.isint ? (take ? c.i : a.i) : 0;
                PUSH(r); break;
            }
            case TG_EXPR_COALESCE: { POP(b); POP(a);
                TVal r; r.isint = a.isint & b.isint;
                r.null = a.null & b.null;
                r.f = a.null ? b.f : a.f;
                r.i = r.isint ? (a.null ? b.i : a.i) : 0;
                PUSH(r); break;
            }
            case TG_EXPR_CONST_NULL: { TVal v; v.f = 0.0; v.i = 0; v.isint = in.arg0 == 0; v.null = true; PUSH(v); break; }
            case TG_EXPR_IN_LIST: { POP(a);
                /* branch-free search for the last item <= a over the sorted,
                 * distinct items inline in prog (16-byte stride); the trip
                 * count depends on the list alone, so the wave stays converged.
                 * (double)item is monotone over sorted items, and every
                 * compare with NaN is false: NaN IN (...) is 0 */
                const tg_expr_inst* base = prog + pc + 1;
                for (int len = in.arg0; len > 1;) {
                    int half = len >> 1;
                    bool le = a.isint ? base[half].imm.i64 <= a.i
                                      : (double)base[half].imm.i64 <= a.f;
                    base += le ? half : 0;
                    len -= half;
                }
                bool found = a.isint ? base->imm.i64 == a.i : (double)base->imm.i64 == a.f;
                TVal r; r.isint = true; r.null = a.null;
                r.i = (!a.null && found) ? 1 : 0;
                r.f = (double)r.i; PUSH(r);
                pc += in.arg0;      /* the items */
                break;
            }
            default: break;
        }
    }
    return TOP;
#undef PUSH
#undef POP
#undef TOP
#undef ARITH
#undef CMP
}

/* the filter / project form: every TG_EXPR_COL names a column of `row` */
__device__ static inline TVal eval_expr(const tg_expr_inst* prog, int count,
                                        const KCol* cols, int64_t row)
{
    return eval_expr_cols(prog, count, RowCols{cols, row});
}

/* host-side program checks shared by every operator that takes a tg_expr
 * (ops_filter.hip): opcodes 0..16 and 32..37 and at most IN_LIST_MAX items per
 * list (else TG_ERR_UNSUPPORTED), well-formed IN lists and CONST_NULL lanes, no
 * underflow and one value left (else TG_ERR_INVALID_ARG), at most
 * EXPR_STACK_SLOTS slots (else `too_deep`) */
tg_status check_expr_depth(const tg_expr* e, tg_status too_deep = TG_ERR_UNSUPPORTED);

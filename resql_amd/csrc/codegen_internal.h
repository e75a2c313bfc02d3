// codegen_internal.h - the walker that turns an operator tree into device pipelines: its state and the declarations of its parts.
// The parts, by what they generate: codegen.cpp (the walk: scans, selections, wave compaction, materialisation), codegen_join.cpp (hash-table
// builds and probes), codegen_agg.cpp (the aggregation sinks), codegen_loop.cpp (the tile loop and the kernel around the row function).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <set>
#include <sstream>

#include "engine_internal.h"


namespace rsq {
namespace cg {


struct Sym { std::string var; Type type; };


// ================================================================================================
// expressions -> device code (emitExpression, reference src/ExpressionsJitFlounder.h:1080-1114)
// ================================================================================================
struct ExprGen {
    std::map<std::string, Sym> symbols;     // JitContextFlounder::symbolTable of the current pipeline
    std::map<std::string, int> strWordVars; // string columns whose first words arrive as row-function parameters <var>_w0, _w1 (loaded with the tile): how many
    bool int16Cast = false;                 // rsq_config.compat_flags & RSQ_COMPAT_JIT_INT16_CAST
    std::map<const Expr*, std::string> tabled;      // sub-expressions answered by a truth table over a dictionary-coded column (Walker::dictTablesWithin): their text

    static std::string ctype(const Type& t) {
        switch (t.tag) {
            case RSQ_BIGINT: case RSQ_DECIMAL: return "i64";
            case RSQ_INT: case RSQ_DATE: return "i32";
            case RSQ_BOOL: return "u8";
            case RSQ_CHAR: return t.len == 1 ? "u8" : "rsq::Str";
            case RSQ_VARCHAR: return "rsq::Str";
            default: failType("no device type for " + serializeType(t));
        }
    }
    static std::string lit64(int64_t v) {
        if (v == INT64_MIN) return "((i64)0x8000000000000000ull)";
        return "((i64)" + std::to_string((long long)v) + "ll)";
    }
    static std::string cstring(const std::string& s) {
        std::string o = "\"";
        for (unsigned char c : s) {
            char buf[8];
            if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
            else if (c < 32 || c > 126) { snprintf(buf, sizeof buf, "\\%03o", c); o += buf; }
            else o += (char)c;
        }
        return o + "\"";
    }
    static int64_t pow10(int n) { int64_t v = 1; while (n-- > 0) v *= 10; return v; }

    std::string constant(const Expr* e) {
        switch (e->type.tag) {
            case RSQ_DECIMAL: case RSQ_BIGINT: return lit64(e->ival);
            case RSQ_INT: case RSQ_DATE: return "((i32)" + std::to_string((long long)(int32_t)e->ival) + ")";
            case RSQ_BOOL: return "((u8)" + std::to_string((int)(uint8_t)e->ival) + ")";
            case RSQ_CHAR:
                if (e->type.len == 1) return "((u8)" + std::to_string((int)(uint8_t)e->ival) + ")";
                [[fallthrough]];
            case RSQ_VARCHAR: return "rsq::str(" + cstring(e->symbol) + ", " + std::to_string(e->type.len) + ")";
            default: failType("Constant code generation not implemented for datatype");
        }
    }

    std::string emit(Expr* e) {
        if (e->type.tag == RSQ_NT) failType("Expression type undefined in emitExpression(..). Have you derived the expression types?");
        auto it = symbols.find(expressionName(e));
        if (it != symbols.end()) return it->second.var;          // value already available under this name
        if (!tabled.empty()) { auto tb = tabled.find(e); if (tb != tabled.end()) return tb->second; }
        switch (e->structure) {
            case LITERAL:
                if (e->tag == RSQ_E_ATTRIBUTE) failType("attribute " + e->symbol + " is not available in this pipeline");
                if (e->tag == RSQ_E_CONSTANT) return constant(e);
                if (e->tag == RSQ_E_STAR) return "((i64)0)";
                failType(std::string("emitExpressionLiteral(..) not implemented for expression type") + exprTagNames[e->tag]);
            case UNARY: return emitUnary(e);
            case BINARY: return emitBinary(e);
            case OTHER: return emitCase(e);
            default: failType("emitExpression(..)");
        }
    }

    std::string emitUnary(Expr* e) {
        if (e->tag == RSQ_E_COUNT) {
            // emitCount: every row counts.  The reference still emits the argument first (emitExpressionUnary,
            // ExpressionsJitFlounder.h:925-928), so an argument it cannot compile refuses the whole plan: emit it for
            // its checks and drop the text.
            if (e->child && e->child->tag != RSQ_E_STAR) (void)emit(e->child);
            return "((i64)1)";
        }
        std::string c = emit(e->child);
        const Type from = e->child->type, to = e->type;
        switch (e->tag) {
            case RSQ_E_SUM: case RSQ_E_AVG: case RSQ_E_MIN: case RSQ_E_MAX: case RSQ_E_AS: return c;
            case RSQ_E_TYPECAST:
                if (to.tag == RSQ_DECIMAL) {
                    if (from.tag == RSQ_DECIMAL) {
                        if (to.scale == from.scale) return c;
                        int d = to.scale - from.scale;
                        if (d > 8 || d < -8) failType("typecast beyond the supported scale difference");
                        if (d > 0) return "rsq::mul(" + c + ", " + lit64(pow10(d)) + ")";
                        return "((i64)((" + c + ") / " + lit64(pow10(-d)) + "))";
                    }
                    if (from.tag == RSQ_BIGINT) {
                        if (to.scale > 8) failType("typecast beyond the supported scale");
                        return "rsq::mul(" + c + ", " + lit64(pow10(to.scale)) + ")";
                    }
                    failType("emitTypecastToDECIMAL(..) code generation not implemented for datatype");
                }
                if (to.tag == RSQ_BIGINT) {
                    // INT -> BIGINT is a 32 -> 64 sign extension (ExpressionsJitFlounder.h:818-824 `movsx`).  The reference's
                    // asmjit back end encodes the 16-bit movsx for it, so its JIT extends the low 16
                    // bits; rsq_config.compat_flags & RSQ_COMPAT_JIT_INT16_CAST reproduces exactly that for hosts that need the JIT's answers.
                    if (from.tag == RSQ_INT) return int16Cast ? "((i64)(short)(" + c + "))" : "((i64)(" + c + "))";
                    if (from.tag == RSQ_DECIMAL) {
                        if (from.scale > 8) failType("typecast beyond the supported scale");
                        return "((i64)((" + c + ") / " + lit64(pow10(from.scale)) + "))";
                    }
                    if (from.tag == RSQ_BIGINT) return c;
                    failType("emitTypecastToBIGINT(..) code generation not implemented for datatype");
                }
                failType("emitTypecast(..) code generation not implemented for datatype");
            default:
                failType(std::string("emitExpression(..) not implemented for expression type") + exprTagNames[e->tag]);
        }
    }

    std::string emitBinary(Expr* e) {
        std::string l = emit(e->child), r = emit(e->child->next);
        const Type res = e->type, op = e->child->type;
        auto arithOk = [&]() {
            if (res.tag != RSQ_DECIMAL && res.tag != RSQ_BIGINT)
                failType(std::string(exprTagNames[e->tag]) + " code generation not implemented for datatype");
        };
        auto orderedOk = [&]() {
            // the reference's own words (ExpressionsJitFlounder.h: emitLessThan says LESS_THAN, emitGreaterThan says ADD)
            const char* name = e->tag == RSQ_E_LT ? "LESS_THAN" : e->tag == RSQ_E_GT ? "ADD" : exprTagNames[e->tag];
            if (op.tag != RSQ_DECIMAL && op.tag != RSQ_DATE && op.tag != RSQ_BIGINT)
                failType(std::string(name) + " code generation not implemented for datatype");
        };
        // string = constant: word-wise against the constant's bytes (rsq_device.h ld_bytes) instead of the byte loop
        auto equalsConstant = [&](bool charSemantics) -> std::string {
            Expr* lc = e->child; Expr* rc = e->child->next;
            const bool lConst = lc->tag == RSQ_E_CONSTANT, rConst = rc->tag == RSQ_E_CONSTANT;
            if (lConst == rConst || !lc->type.isString() || !rc->type.isString() || 1 == 0) return "";
            const Expr* cst = lConst ? lc : rc;
            const std::string& x = lConst ? r : l;
            const int cap = (lConst ? rc : lc)->type.len;
            std::string text = cst->symbol;
            if (text.find('\0') != std::string::npos) return "";
            if (charSemantics) while (!text.empty() && text.back() == ' ') text.pop_back();
            if ((int)text.size() > cap) return "((u8)0)";            // longer than any value of the column
            std::string cond, condRest;          // (condRest: the words behind the prefetched ones - fetched only if those match)
            const int nPre = strWordVars.count(x) ? strWordVars[x] : 0;
            for (int w = 0; w * 8 < cap; w++) {
                const int rbytes = std::min(8, cap - w * 8);
                uint64_t cw = 0, mask = 0;
                for (int i = 0; i < rbytes; i++) {
                    const size_t k = (size_t)(w * 8 + i);
                    if (k < text.size()) { cw |= (uint64_t)(uint8_t)text[k] << (8 * i); mask |= 0xFFull << (8 * i); }
                    else mask |= (charSemantics ? 0xDFull : 0xFFull) << (8 * i);
                }
                char buf[200];
                if (w < nPre) snprintf(buf, sizeof buf, "((%s_w%d ^ 0x%llxull) & 0x%llxull)", x.c_str(), w, (unsigned long long)cw, (unsigned long long)mask);
                else
                snprintf(buf, sizeof buf, "((rsq::ld_bytes<%d>((%s).p + %d) ^ 0x%llxull) & 0x%llxull)", rbytes, x.c_str(), w * 8,
                         (unsigned long long)cw, (unsigned long long)mask);
                std::string& into = nPre > 0 && w >= nPre ? condRest : cond;
                into += (into.empty() ? "" : " | ") + std::string(buf);
            }
            if (!condRest.empty()) return "((u8)(((" + cond + ") == 0ull) && ((" + condRest + ") == 0ull)))";
            return "((u8)((" + cond + ") == 0ull))";
        };
        auto equals = [&]() -> std::string {
            if (op.tag == RSQ_VARCHAR || (op.tag == RSQ_CHAR && op.len > 1)) {
                const std::string fast = equalsConstant(op.tag == RSQ_CHAR);
                if (!fast.empty()) return fast;
            }
            switch (op.tag) {
                case RSQ_DECIMAL: case RSQ_INT: case RSQ_BIGINT: case RSQ_BOOL: case RSQ_DATE:
                    return "((u8)((" + l + ") == (" + r + ")))";
                case RSQ_CHAR:
                    if (op.len > 1) return "rsq::compare_char(" + l + ", " + r + ")";
                    return "((u8)((" + l + ") == (" + r + ")))";
                case RSQ_VARCHAR: return "rsq::compare_varchar(" + l + ", " + r + ")";
                default: failType("EQUALS code generation not implemented for datatype");
            }
        };
        switch (e->tag) {
            case RSQ_E_ADD: arithOk(); return "rsq::add(" + l + ", " + r + ")";
            case RSQ_E_SUB: arithOk(); return "rsq::sub(" + l + ", " + r + ")";
            case RSQ_E_MUL: arithOk(); return "rsq::mul(" + l + ", " + r + ")";
            case RSQ_E_DIV: arithOk(); return "rsq::div(" + l + ", " + r + ", a.err)";
            case RSQ_E_AND: return "((u8)((" + l + ") & (" + r + ")))";      // no short circuit, as in the reference
            case RSQ_E_OR: return "((u8)((" + l + ") | (" + r + ")))";
            case RSQ_E_LT: orderedOk(); return "((u8)((" + l + ") < (" + r + ")))";
            case RSQ_E_LE: orderedOk(); return "((u8)((" + l + ") <= (" + r + ")))";
            case RSQ_E_GT: orderedOk(); return "((u8)((" + l + ") > (" + r + ")))";
            case RSQ_E_GE: orderedOk(); return "((u8)((" + l + ") >= (" + r + ")))";
            case RSQ_E_EQ: return equals();
            case RSQ_E_NEQ: return "((u8)(1 - " + equals() + "))";
            case RSQ_E_LIKE: {
                // emitLike passes both operands to stringLikeCheck as char* (ExpressionsJitFlounder.h:695-705): a CHAR(1)
                // operand is a byte there, not a pointer — undefined in the reference, refused here
                const Type rt = e->child->next->type;
                if (!op.isString() || !rt.isString()) failType("LIKE on a CHAR(1) operand is undefined in the reference");
                return "rsq::like(" + l + ", " + r + ")";
            }
            default: failType(std::string("emitExpressionBinary(..) not implemented for expression type") + exprTagNames[e->tag]);
        }
    }

    // ---- arithmetic typed by value range (the register aggregation over narrow scan columns, codegen_agg.cpp) ----
    // A scan column read from a narrow image has an ENVELOPE from its statistics: a sign class (min >= 0 or not) and the bit width of
    // max(|min|, |max|) - a power of two, never the values, so one plan shape keeps one text across scale factors and bases.  Where the
    // envelope fits 31 bits the column reaches the row function as an i32 (typedLeaves: the i64 name other consumers read -> that
    // parameter), and +, -, * over such leaves and constants are emitted at the width their own envelope proves: the exact result is
    // then representable, so it IS the wrapped i64 result of rsq::add / sub / mul.  Everything else widens its operands and is
    // emitted as before.
    struct TypedLeaf { std::string narrow; bool neg; int bits; };
    std::map<std::string, TypedLeaf> typedLeaves;
    struct TV { std::string text; bool is32 = false, known = false; __int128 lo = 0, hi = 0; };
    static std::string wide(const TV& v) { return v.is32 ? "((i64)(" + v.text + "))" : v.text; }
    static TV constantTV(int64_t v) {
        TV t; t.known = true; t.lo = t.hi = v;
        t.is32 = v > -(int64_t(1) << 31) && v < (int64_t(1) << 31);
        t.text = t.is32 ? "((i32)" + std::to_string((long long)v) + ")" : lit64(v);
        return t;
    }
    TV arithTV(int tag, const TV& a, const TV& b) {
        const __int128 M31 = ((__int128)1 << 31) - 1, M63 = ((__int128)1 << 63) - 1;
        TV r;
        if (a.known && b.known) {
            if (tag == RSQ_E_ADD) { r.lo = a.lo + b.lo; r.hi = a.hi + b.hi; }
            else if (tag == RSQ_E_SUB) { r.lo = a.lo - b.hi; r.hi = a.hi - b.lo; }
            else {
                const __int128 p[4] = {a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi};
                r.lo = *std::min_element(p, p + 4); r.hi = *std::max_element(p, p + 4);
            }
            r.known = r.lo >= -M63 && r.hi <= M63;
            if (r.known && r.lo == r.hi) return constantTV((int64_t)r.lo);      // (constants fold: `1` as DECIMAL(.., 2) is 100)
        }
        const char* op = tag == RSQ_E_ADD ? " + " : tag == RSQ_E_SUB ? " - " : " * ";
        if (r.known && a.is32 && b.is32) {
            if (r.lo >= -M31 && r.hi <= M31) {
                r.is32 = true;
                const __int128 U24 = ((__int128)1 << 24) - 1, S24 = ((__int128)1 << 23) - 1;
                if (tag == RSQ_E_MUL && a.lo >= 0 && b.lo >= 0 && a.hi <= U24 && b.hi <= U24)
                    r.text = "((i32)__umul24((u32)(" + a.text + "), (u32)(" + b.text + ")))";
                else if (tag == RSQ_E_MUL && a.lo >= -S24 && b.lo >= -S24 && a.hi <= S24 && b.hi <= S24)
                    r.text = "__mul24(" + a.text + ", " + b.text + ")";
                else r.text = "(" + a.text + op + b.text + ")";
            } else if (tag == RSQ_E_MUL && a.lo >= 0 && b.lo >= 0)        // widening 32 x 32 -> 64, by the sign classes
                r.text = "((i64)((u64)(u32)(" + a.text + ") * (u64)(u32)(" + b.text + ")))";
            else r.text = "((i64)(" + a.text + ")" + op + "(i64)(" + b.text + "))";
            return r;
        }
        r.text = std::string(tag == RSQ_E_ADD ? "rsq::add(" : tag == RSQ_E_SUB ? "rsq::sub(" : "rsq::mul(") + wide(a) + ", " + wide(b) + ")";
        return r;
    }
    // +, -, * over attributes, constants and casts alone: what emitTyped follows.  Anything else in an input (a CASE, whose conditions
    // may be answered by truth tables that exist only while the input is first emitted) keeps the text it has.
    bool pureArithmetic(const Expr* e) {
        if (symbols.count(expressionName(e))) return true;
        if (e->structure == LITERAL) return e->tag == RSQ_E_CONSTANT;
        if (e->structure == UNARY) return (e->tag == RSQ_E_SUM || e->tag == RSQ_E_AS || e->tag == RSQ_E_TYPECAST) && e->child && pureArithmetic(e->child);
        if (e->structure == BINARY) return (e->tag == RSQ_E_ADD || e->tag == RSQ_E_SUB || e->tag == RSQ_E_MUL) && pureArithmetic(e->child) && pureArithmetic(e->child->next);
        return false;
    }
    TV emitTyped(Expr* e) {
        TV v;
        auto untyped = [&]() { v.text = emit(e); return v; };
        auto it = symbols.find(expressionName(e));
        if (it != symbols.end()) {
            auto tl = typedLeaves.find(it->second.var);
            if (tl == typedLeaves.end()) return untyped();
            v.text = tl->second.narrow; v.is32 = v.known = true;
            v.hi = ((__int128)1 << tl->second.bits) - 1; v.lo = tl->second.neg ? -v.hi : 0;
            return v;
        }
        if (!tabled.empty() && tabled.count(e)) return untyped();
        const bool arith = e->type.tag == RSQ_DECIMAL || e->type.tag == RSQ_BIGINT;
        if (e->structure == LITERAL && e->tag == RSQ_E_CONSTANT && arith) return constantTV(e->ival);
        if (e->structure == UNARY && e->child && e->tag != RSQ_E_COUNT) {
            const Type from = e->child->type, to = e->type;
            if (e->tag == RSQ_E_SUM || e->tag == RSQ_E_AS) return emitTyped(e->child);
            if (e->tag == RSQ_E_TYPECAST && to.tag == RSQ_DECIMAL && (from.tag == RSQ_DECIMAL || from.tag == RSQ_BIGINT)) {
                const int d = to.scale - (from.tag == RSQ_DECIMAL ? from.scale : 0);
                if (d == 0) return emitTyped(e->child);      // (BIGINT -> DECIMAL(.., 0) is a multiplication by 1)
                if (d > 0 && d <= 8) return arithTV(RSQ_E_MUL, emitTyped(e->child), constantTV(pow10(d)));
            }
            return untyped();
        }
        if (e->structure == BINARY && arith && (e->tag == RSQ_E_ADD || e->tag == RSQ_E_SUB || e->tag == RSQ_E_MUL))
            return arithTV(e->tag, emitTyped(e->child), emitTyped(e->child->next));
        return untyped();
    }

    std::string emitCase(Expr* e) {   // ExpressionsJitFlounder.h:720-754
        std::string out, close;
        Expr* c = e->child;
        for (; c && c->tag == RSQ_E_WHENTHEN; c = c->next) {
            out += "((" + emit(c->child) + ") ? (" + emit(c->child->next) + ") : ";
            close += ")";
        }
        if (c) out += "(" + emit(c) + ")";
        else out += (e->type.isString() ? std::string("rsq::str(\"\", 0)") : "((" + ctype(e->type) + ")0)");
        return out + close;
    }
};

// value of a 64-bit table word as a typed device value, and back
inline std::string fromWord(const std::string& w, const Type& t) {
    switch (t.tag) {
        case RSQ_BIGINT: case RSQ_DECIMAL: return w;
        case RSQ_INT: case RSQ_DATE: return "((i32)(" + w + "))";
        case RSQ_BOOL: return "((u8)(" + w + "))";
        case RSQ_CHAR: if (t.len == 1) return "((u8)(" + w + "))"; [[fallthrough]];
        case RSQ_VARCHAR: return "rsq::str_from_addr(" + w + ", " + std::to_string(t.len) + ")";     // payload strings travel by address
        default: failUnsupported("value type cannot be carried in a hash table word");
    }
}
inline std::string toWord(const std::string& v, const Type& t) {
    // a string is carried as the device address of its bytes in the (immutable, device-resident) column it comes from
    if (t.isString()) return "rsq::str_addr(" + v + ")";
    return "((i64)(" + v + "))";
}

// ================================================================================================
// the walk
// ================================================================================================
struct Walker {
    Query& q;
    ExprGen eg;

    // state of the pipeline under construction
    Pipeline pipe;
    std::vector<std::string> colTypes;        // device type per scanned (vector-loadable) column
    std::vector<int> colIsString;
    std::vector<int> colNarrow;               // per scanned column: the byte width of the narrow image it is read from (0: the wide column)
    // a scanned column's value in row `r` / a lane's two rows of it into `dst`: decoded where the column is read from its narrow image
    std::string colAt(int k, const std::string& r) const {
        const std::string K = std::to_string(k);
        if (k < (int)colNarrow.size() && colNarrow[(size_t)k]) return "rsq::dec<" + colTypes[(size_t)k] + ">(a.c" + K + "[" + r + "], a.fb" + K + ")";
        return "a.c" + K + "[" + r + "]";
    }
    std::string tileLoad(int k, const std::string& dst) const {
        const std::string K = std::to_string(k);
        if (k < (int)colNarrow.size() && colNarrow[(size_t)k]) return "rsq::ld2n(a.c" + K + " + b, a.fb" + K + ", " + dst + ");";
        return "rsq::ld2(a.c" + K + " + b, " + dst + ");";
    }
    // Dictionary-coded string columns (engine.h TableColumn::dict): per scanned column the width W of its values, 0 = not coded.  The scan
    // treats such a column as a one-byte tile column (colIsString 0, colTypes "u8") whose row-function parameter is the code, vc_<k>;
    // the row function's first lines turn it into the rsq::Str v_<k> that points into the dictionary (a.d<k>, a kernel argument).
    std::vector<int> colDict;
    // Scan columns the register aggregation decodes as i32 (typeScanColumns, codegen_agg.cpp): the row function's parameter is n_<k>, and
    // its first lines widen it into the i64 v_<k> every consumer that is not typed reads.
    std::vector<char> colTyped;
    bool typedCol(int k) const { return k >= 0 && k < (int)colTyped.size() && colTyped[(size_t)k] != 0; }
    static bool envelopeOf(const TableColumn& c, bool& neg, int& bits);
    bool typeScanColumns();
    bool coded(int k) const { return k >= 0 && k < (int)colDict.size() && colDict[(size_t)k] != 0; }
    std::string paramName(int k) const { return (coded(k) ? "vc_" : typedCol(k) ? "n_" : "v_") + std::to_string(k); }
    std::string dictDecode(int k, const std::string& code) const {
        const std::string K = std::to_string(k), W = std::to_string(colDict[(size_t)k]);
        return "rsq::str(a.d" + K + " + (u32)(" + code + ") * " + W + "u, " + W + ")";
    }
    // Truth tables: a boolean expression whose only non-constant leaf is ONE coded column is evaluated once per dictionary entry in the kernel's
    // prologue - by the expression text the row function would have run - and a row tests bit `code` of the 256-bit result (LDS, s_dt).
    int nDictTables = 0;
    int dictTableColumn(const Expr* e, int col = -1);       // the coded column e depends on alone (-1: none, -2: does not qualify)
    void dictTablesWithin(Expr* e);                         // registers them in eg.tabled; the caller clears it behind its emit
    int storedWidth(int k) const {            // bytes per row the scan fetches of column k (non-string)
        if (k < (int)colNarrow.size() && colNarrow[(size_t)k]) return colNarrow[(size_t)k];
        return colTypes[(size_t)k] == "i64" ? 8 : colTypes[(size_t)k] == "i32" ? 4 : 1;
    }
    std::string rowParams, rowArgsTail, rowArgsTailGuarded;
    // key-bitmap words fetched for both rows of a lane (and all tiles in flight) before the first row is processed:
    // (table name, scanned column index) — see consumeProbe
    struct BitmapPrefetch { std::string first; int second; bool interleaved; };
    std::vector<BitmapPrefetch> bitmapPrefetch;
    std::string body;                          // row function body
    std::string closers;                       // closing braces of the open scopes
    std::string stateDecl, stateInit, prologue, epilogue, fileScope;
    std::string helperFns;                     // device functions behind Args / State, in front of the row function
    std::vector<std::string> explainSteps;
    int indent = 1;
    int matchSlotTable = -1;                   // innermost single-match probe whose slot variable is in scope
    std::map<int, std::string> slotVar;        // hash table id -> device variable holding the matched slot
    std::map<std::string, int> symbolOrigin;   // symbol -> hash table id it was read from (or -1: scan column)
    std::map<std::string, int> symbolWord;     // symbol -> word index in that table
    bool multiMatchAbove = false;
    std::string repeatedKeysAbove;             // a probe for all matches above whose table's build keys repeat for certain (HashTable::dupKeysKnown): which
    std::string denseRefusal;                  // RSQ_DICT_SCANS=2: why a string group key did not become a dense id (tryDenseKeys), for explain
    bool underNestedLoops() const { return !q.nljs.empty(); }      // the plan pairs rows in a nested-loops join
    // wave-level compaction (see compactThen)
    bool selective = false, compacted = false;
    // the selection directly above the scan: its text over the row's column variables, the columns it reads and the fraction of
    // rows it is expected to pass (column statistics, values taken as uniform) - the late-load form of the tile loop (below)
    std::string leadCond; std::vector<int> leadCols; double leadPass = 1.0;
    std::string stage2Prefix;               // necessary conditions of later joins, tested at the top of stage 2 (consumeProbe: component bitmaps)
    struct CompFilter { std::string table, symbol, stage2Var; int64_t bits; };
    std::vector<CompFilter> compFilters;    // ... as consumeProbe found them while stage 2 was generated
    bool inStage2 = false;                  // the walk is generating the code behind the wave compaction
    bool leadPassComplete = true;       // every part of the predicate was understood (else the estimate is an upper bound only)
    // the selection directly above the scan, as text: where its scope starts in `body` and its condition (finishPipeline: the count pass of a
    // materialisation evaluates it for both rows of a lane first, "pairCond")
    size_t pairSplit = std::string::npos; std::string pairCond;
    std::string stage2Body;
    std::vector<std::pair<std::string, Sym>> cqLive;     // carried symbols: name -> stage-1 variable and type

    explicit Walker(Query& q_) : q(q_) { eg.int16Cast = jitInt16Cast(q_.ctx); }

    void line(const std::string& s) { body += std::string((size_t)indent * 4, ' ') + s + "\n"; }
    void openScope(const std::string& head) { line(head); indent++; }
    void closeScope() { indent--; line("}"); }
    void addArg(const std::string& name, const std::string& ctype, uint64_t v);

    void produce(OpNode* o, std::vector<std::string> request);

    std::map<OpNode*, std::vector<std::string>> requestOf;
    std::map<OpNode*, int> joinPhase;

    static bool has(const std::vector<std::string>& v, const std::string& s) { return std::find(v.begin(), v.end(), s) != v.end(); }

    Schema prune(const Schema& s, const std::vector<std::string>& req);

    void produceScan(OpNode* o, std::vector<std::string> request);

    bool sideRange(const Expr* e, double& lo, double& hi, int& col);
    double passFraction(const Expr* e);
    void leadColumnsOf(const Expr* e, std::vector<int>& out, bool& ok);
    // Short string columns the selection right above the scan compares with constants: their bytes are loaded WITH the tile (one or
    // two 8-byte words per row, in flight together with the numeric columns) and reach the row function as parameters, instead of
    // being fetched inside it row by row - eight dependent round trips per lane and iteration (TPC-H Q3's customer pipeline:
    // c_mktsegment = 'BUILDING').
    std::vector<std::pair<int, int>> strPrefetch;         // (scanned column, bytes of it that arrive with the tile), in the order of the row function's parameters
    std::map<int, int> strPrefetchWidth;                   // scanned column -> its width (the row stride)
    // Staged string tiles.  A lane that fetches ITS two rows of a CHAR(25) column asks for 8 bytes at a stride of 50: the wave's one load
    // instruction touches 25 memory lines, the next word's the same 25 again, and the texture unit, not the memory, bounds the kernel (TPC-H
    // Q19 at SF10: 63 B rows at 3.5 TB/s, against 6.8 for Q1's plain columns).  A column of at most 32 bytes is therefore fetched as what it
    // is - 128 rows x W contiguous bytes per tile, 16 bytes per lane and load, every line once - and passed through the wave's own LDS
    // region, from which each lane reads its rows' words (ds_read_b64 takes any address on gfx950).  All words of the value then arrive
    // as row-function parameters.
    std::string foldTile;                                  // code behind every tile of the tile loops: the periodic fold of 32-bit partial sums (codegen_agg.cpp)
    int accRegs = 0;                                       // VGPRs the register aggregation's State holds per lane: 2 per i64 accumulator, 1 per partial sum or u32 first row
    // The register aggregation's second form (codegen_agg.cpp, row_cells.h): its text stands between marker lines in stateDecl, prologue, body,
    // foldTile and epilogue until finishPipeline knows whether the statement gets it.  IFNOT ... [ELSE ...] END and IF ... END; no nesting.
    // Whoever transforms one of those five buffers between emitDenseAggregation and resolveRowCells (finishPipeline, right behind the
    // fourWaves decision) must leave the marker lines whole and in order: typeScanColumns, the only one today, prepends to body.  The
    // decision cannot simply move in front of emitDenseAggregation: it reads accRegs and foldTile, which that function makes.
    bool rowCells = false;
    static constexpr const char* RC_IFNOT = "\x01rc-ifnot\n"; static constexpr const char* RC_IF = "\x01rc-if\n";
    static constexpr const char* RC_ELSE = "\x01rc-else\n"; static constexpr const char* RC_END = "\x01rc-end\n";
    static void resolveRowCells(std::string& text, bool keep);
    std::string postTile;                                  // code behind the two row_fn calls of a tile in the tile loops ($TILE = the tile's number; wave-uniform)
    std::map<int, int> strStaged;                          // scanned column -> byte offset of its tile in the wave's LDS region
    int strStagedBytes = 0;                                // bytes of that region (128 x the staged widths)
    void prefetchComparedStrings(const Expr* e);
    void noteLeadingSelection(const Expr* e, const std::string& cond);

    void consume(OpNode* o, OpNode* from);

    bool downstreamMaterializes(OpNode* o);
    bool compactThen(OpNode* o, const std::function<void()>& downstream);

    void countPerThread(const std::string& T, bool identityCapable = false);

    std::vector<std::string> keyWords(Expr* e, const std::string& prefix, bool stripChar, std::vector<std::string>* endsWithSpace = nullptr, int stripMode = -1);

    // String join keys of different declared lengths.  The reference hashes each side with its own type: hashVarchar stops
    // at the NUL, so VARCHAR(a) = VARCHAR(b) matches equal strings — both sides take the word count of the wider one, the
    // narrower side's missing words are zero.  hashChar pads with spaces to the DECLARED length (qlib/hash.h:131-147), so
    // CHAR(a) = CHAR(b), a != b, never has equal hashes and never matches: the two sides get pad words that differ.
    // CHAR against VARCHAR (any lengths): equal hashes need the VARCHAR value to be exactly as long as the CHAR column is wide
    // (hashChar counts the pad spaces, hashVarchar only the characters), and the key comparison is the PROBE side's
    // (checkEquality(probeKeys, entryKeys), hashjoin.h:142/191: compareChar ignores trailing spaces, compareVarchar does not).
    // So both sides form their words the probe side's way (joinKeyStripMode), padded to the wider side's word count, plus one
    // word that holds the hashed length: the declared width of a CHAR key, the actual length of a VARCHAR key.
    static bool mixedStringKinds(const Expr* a, const Expr* b) { return a->type.isString() && b->type.isString() && a->type.tag != b->type.tag; }
    static int joinKeyStripMode(const Expr* side, const Expr* probeSide, const Expr* buildSide);
    void padKeyWords(Expr* mine, Expr* other, size_t w0, std::vector<std::string>& keyVars, bool buildSide);

    std::string hashOf(const std::vector<std::string>& keyVars);

    static std::string wordAt(const HashTable& ht, const std::string& T, int w);

    std::string slotOf(const HashTable& ht, const std::string& T, const std::vector<std::string>& keyVars);

    // RSQ_DICT_SCANS=2: where a build-side string's bytes stand, if that is a dictionary image (HashTable::DictOrigin) - a coded column of
    // this pipeline's scan, or a payload of an earlier table that has an origin itself.  Only for a name some aggregation of the statement
    // groups by: every other statement keeps the text it has under RSQ_DICT_SCANS=1.
    bool isGroupKey(const std::string& name) const;
    HashTable::DictOrigin payloadOriginOf(const std::string& name) const;

    void consumeBuild(OpNode* o, OpNode* from);
    void consumeBuildBody(OpNode* o, OpNode* from);

    void probeKeys(OpNode* o, const std::string& T, std::vector<std::string>& keyVars, std::vector<std::string>& probeKeyNames);

    void consumeProbe(OpNode* o, OpNode* from);

    void consumeMatch(OpNode* o, HashTable& ht, const std::string& T, const std::vector<std::string>& keyVars,
                      const std::vector<std::string>& probeKeyNames);

    void probeTable(OpNode* o, HashTable& ht, const std::string& T, const std::vector<std::string>& keyVars,
                    const std::vector<std::string>& probeKeyNames);
    std::map<std::string, std::pair<int, int>> probeKeyOf;   // probe-side key symbol -> (table, key word)
    // the join probes whose match is in scope (innermost last): table, single match?, the probe side's key symbols ("" where a key
    // is not a one-word attribute) — emitHashAggregation's functional dependencies
    struct ProbeInScope { int table; bool single; bool rankCapable; std::vector<std::string> keySymbols; };
    std::vector<ProbeInScope> probesInScope;

    void collectAccumulators(OpNode* o);

    bool tryDenseKeys(OpNode* o);
    std::string stage2Code(int k);          // stage-2 name of the code of dictionary-coded scan column k (codegen.cpp)

    bool tryJoinEntry(OpNode* o);

    void consumeAggregation(OpNode* o, OpNode* from);

    void emitHashAggregation(OpNode* o);

    std::string groupIdExpr();

    static const char* identityOf(int merge) { return merge == 0 ? "0ull" : merge == 2 ? "0x7fffffffffffffffull" : "0x8000000000000000ull"; }

    std::string blockIdentityExpr(const std::string& blk);

    void emitGlobalFlush(std::ostringstream& s, const std::string& count, const std::string& srcExpr, int64_t D, int stride = 1);

    void emitStagedScatter(int64_t D, int W, int gpp, int shift, int P);

    void emitDenseAggregation(OpNode* o);

    void emitJoinEntryAggregation(OpNode* o);

    void consumeMaterialize(OpNode* o, OpNode* from);
    void consumeNestedLoops(OpNode* o, OpNode* from);
    bool nestedLoopsFeedsAggregation(OpNode* o, bool& probesAbove);      // the rows above join `o` end in this pipeline's aggregation (... through a probe or another pair loop)

    std::string postTileFor(const std::string& tile);
    int stagedRounds(int col) { return (8 * strPrefetchWidth[col] + 63) / 64; }
    void stagedChunkDecls(std::ostringstream& s, const std::string& ind, const char* pre, int col, int u) {
        for (int r = 0; r < stagedRounds(col); r++) s << ind << "rsq::u32v4 " << pre << col << "_" << u << "_" << r << " = {0u, 0u, 0u, 0u};\n";
    }
    void stagedChunkLoads(std::ostringstream& s, const std::string& ind, const char* pre, int col, int u);
    void stagedUnstage(std::ostringstream& s, const std::string& ind, int u);

    void emitLateLoads(std::ostringstream& s, const std::string& tile, int u, const std::vector<char>& lateCol, const std::string& tileEnd = "ntiles");

    void finishPipeline();
};

}  // namespace cg
}  // namespace rsq

// rowstore.cpp — the row-store bridge on the host (rsq_table_from_rowstore's default path): packed ReSQL tuples (strings by value,
// schema.h:76-106 offsets) transposed into columns by one host thread.  The cell rule is rowstore.h's, shared with the device path.
#include "rowstore.h"

namespace rsq {

RowstoreLayout rowstoreLayout(const std::vector<Type>& types) {
    RowstoreLayout l;
    for (const Type& t : types) { l.offset.push_back(l.tupleSize); l.tupleSize += sizeInTuple(t, true); }
    for (const Type& t : types) {
        l.width.push_back(columnWidth(t));
        l.category.push_back(t.tag == RSQ_CHAR || t.tag == RSQ_VARCHAR ? rowst::CAT_STRING : rowst::CAT_NUMERIC);
    }
    return l;
}

int64_t rowstoreRows(const size_t* contentSize, int32_t nBlocks, int tupleSize) {
    int64_t n = 0;
    for (int b = 0; b < nBlocks; b++) n += (int64_t)(contentSize[b] / (size_t)tupleSize);
    return n;
}

void transposeRowstoreHost(const std::vector<Type>& types, const uint8_t* const* blocks, const size_t* contentSize, int32_t nBlocks,
                           std::vector<std::vector<uint8_t>>& cols, int64_t& n) {
    const RowstoreLayout l = rowstoreLayout(types);
    const int nCols = (int)types.size(), ts = l.tupleSize;
    n = rowstoreRows(contentSize, nBlocks, ts);
    cols.assign((size_t)nCols, std::vector<uint8_t>());
    for (int i = 0; i < nCols; i++) cols[(size_t)i].assign((size_t)n * (size_t)l.width[(size_t)i], 0);
    int64_t r = 0;
    for (int b = 0; b < nBlocks; b++) {
        size_t cnt = contentSize[b] / (size_t)ts;
        for (size_t k = 0; k < cnt; k++, r++) {
            const uint8_t* tup = blocks[b] + k * (size_t)ts;
            for (int i = 0; i < nCols; i++) {
                int w = l.width[(size_t)i];
                uint8_t* dst = cols[(size_t)i].data() + (size_t)r * (size_t)w;
                rowst::cell(l.category[(size_t)i], w, tup + l.offset[(size_t)i], dst);
            }
        }
    }
}

}  // namespace rsq

// tbl.h — what "a line" of a '.tbl' file is (tbl.cpp): the one definition both ingest paths use.  The host path (parseTblFile) calls
// tblParseLine for every line; the device path (tbl_device.hip) parses the plain forms of tbl_fields.h itself and hands every other
// line to the same function, so error texts and accepted oddities are the host path's by construction.  No device code, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "expr.h"

namespace rsq {

// One line -> one cell per column.  `line` holds `len` bytes without the '\n' and is writable INCLUDING line[len] (fields are NUL
// terminated in place while they are parsed; every byte is put back).  cells[i]: columnWidth(types[i]) zero bytes.  Returns null, or
// the text that follows "Line N in <path> " (it lives in `what`): "contains extra attributes.", "field K: <reason>",
// "is missing attributes.".  Cells in front of the failing field are written.
const char* tblParseLine(const std::vector<Type>& types, char* line, size_t len, char terminator, uint8_t* const* cells, std::string& what);

// '.tbl' text -> columns (columnWidth(type) bytes per row) and the row count, with the reference's BULK INSERT semantics
// (execute.h:332-388)
void parseTblFile(const std::string& path, const std::vector<Type>& types, char terminator, int nThreads,
                  std::vector<std::vector<uint8_t>>& cols, int64_t& nRows);

}  // namespace rsq

"""Device BULK INSERT cases (tests/test_gpu_tbl_device.py): the seam shapes - file sizes, line counts, long lines and odd lines at the
boundaries of the kernels' 4096-byte text blocks, 256-line workgroups and LDS tile - as bytes, for a one-column and a three-column
schema.  Every shape is a pure function of its name: the files are written by the test that loads them."""
from resql_amd import plan as P

T = P.TypeInit
BLOCK = 4096          # csrc/tbl_device.hip TBL_BLOCK_BYTES
GROUP = 256           # ... TBL_GROUP_LINES
TILE = 49152          # ... TBL_TILE_BYTES

S1 = P.Table("s1", [P.Column("i", T.INT())], 0)
S3 = P.Table("s3", [P.Column("i", T.INT()), P.Column("c", T.CHAR(5)), P.Column("d", T.DECIMAL(12, 2))], 0)
SCHEMAS = {"s1": S1, "s3": S3}


def plain_line(kind: str, k: int, width: int = 0) -> str:
    """a plain line of row k; width > 0: exactly that many bytes (s1: 1..9, s3: 13..21), by the digits of the INT field"""
    if kind == "s1":
        digits = width or 7
        tail = ""
    else:
        tail = f"|r{k % 1000:03d}|-{k % 10}.{k % 100:02d}|"          # 12 bytes: "|rNNN|-N.NN|"
        digits = (width - len(tail)) if width else 3
    assert 1 <= digits <= 9, (kind, width)
    return str(10 ** (digits - 1) + k % (9 * 10 ** (digits - 1))) + tail


def odd_line(kind: str, k: int) -> str:
    """a line the device hands to the host, which accepts it: a leading blank and a sign"""
    return f" {k + 1}" if kind == "s1" else f" {k + 1}|odd{k % 10}|+{k % 7}.5|"


def fill(kind: str, total: int, first: int = 0) -> list:
    """plain lines of rows first.. whose bytes, a '\\n' behind every one of them, are exactly `total`"""
    base = 7 if kind == "s1" else 16
    per = base + 1
    n, rem = divmod(total, per)
    assert n >= 1 and rem <= 2 * n, (total, n, rem)          # (every line can grow by two bytes)
    return [plain_line(kind, first + i, base + (1 if i < rem else 0) + (1 if i < rem - n else 0)) for i in range(n)]


def lines_of(kind: str, shape: str) -> list:
    """the lines of a shape (without line ends)"""
    if shape == "empty":
        return []
    if shape == "one_line":
        return [plain_line(kind, 0)]
    if shape == "exactly_one_block":          # BLOCK bytes with the final '\n' (content() makes the file without it BLOCK bytes too)
        return fill(kind, BLOCK)
    if shape == "newline_ends_block_0":       # a '\n' at byte BLOCK - 1, rows behind it
        head = fill(kind, BLOCK)
        return head + [plain_line(kind, len(head) + i) for i in range(5)]
    if shape == "newline_starts_block_1":     # a '\n' at byte BLOCK
        head = fill(kind, BLOCK + 1)
        return head + [plain_line(kind, len(head) + i) for i in range(5)]
    if shape.startswith("lines_"):            # around the workgroup's 256 lines
        return [plain_line(kind, i) for i in range(int(shape[6:]))]
    if shape == "long_line":                  # 9 000 bytes over three blocks, between short rows
        if kind == "s1":
            long = "0" * 8995 + "12345"       # odd (more than 9 digits); the host reads 12345
        else:
            long = "77|" + "abcdefghij" * 899 + "|3.25|"          # the CHAR(5) field keeps "abcde"
        assert 8990 <= len(long) <= 9010
        return [plain_line(kind, 0), plain_line(kind, 1), long, plain_line(kind, 3)]
    if shape == "span_exceeds_tile":          # 256 lines of 300 bytes: the workgroup reads global memory
        if kind == "s1":
            rows = ["0" * 291 + f"{100000000 + i}" for i in range(GROUP)]
        else:
            rows = [f"{i + 1}|" + ("q%03d" % i) * 72 + "|1.25|" for i in range(GROUP)]
        assert all(295 <= len(r) <= 300 for r in rows) and sum(len(r) + 1 for r in rows) > TILE
        return rows + [plain_line(kind, 999)]
    if shape == "odd_first":
        return [odd_line(kind, 0)] + [plain_line(kind, i) for i in range(1, 40)]
    if shape == "odd_last":
        return [plain_line(kind, i) for i in range(39)] + [odd_line(kind, 39)]
    if shape == "odd_across_block":           # the odd line starts in block 0 and ends in block 1
        head = fill(kind, BLOCK - 3)
        return head + [odd_line(kind, len(head))] + [plain_line(kind, len(head) + 1 + i) for i in range(3)]
    if shape == "crlf":                       # the '\r' joins the last field: odd, and the host reads the number in front of it
        return [(plain_line(kind, i) if kind == "s1" else plain_line(kind, i)[:-1]) + "\r" for i in range(6)]
    if shape == "crlf_after_terminator":      # s3: behind a trailing terminator the '\r' is one field too many (s1: a field of its own)
        return [(plain_line(kind, i) + ("|" if kind == "s1" else "")) + "\r" for i in range(6)]
    raise KeyError(shape)


SHAPES = ["empty", "one_line", "exactly_one_block", "newline_ends_block_0", "newline_starts_block_1",
          "long_line", "lines_255", "lines_256", "lines_257", "lines_513", "span_exceeds_tile",
          "odd_first", "odd_last", "odd_across_block", "crlf", "crlf_after_terminator"]


def content(kind: str, shape: str, final_newline: bool) -> bytes:
    lines = fill(kind, BLOCK + 1) if shape == "exactly_one_block" and not final_newline else lines_of(kind, shape)
    return ("\n".join(lines) + ("\n" if final_newline else "")).encode()          # ("empty" with a final newline: one empty line)

"""The kernel that packs a materialisation's columns into ReSQL tuples (resql_amd/csrc/result_pack.hip k_pack_tuples) through
rsq_prim_pack_tuples, against a numpy restatement of the tuple's bytes written here - never against the engine.  A workgroup takes
R = min(256, 48 KiB / tuple size) rows and assembles their span in LDS; the row counts sit on both sides of R and of two workgroups, the
tuple sizes make spans start at every alignment, and one tuple is longer than the tile (R = 0: the path through global memory).  The device
buffer is filled with 0xEE before the launch and carries 64 guard bytes behind the tuples: every byte of the tuples must equal the
restatement (so none is left unwritten) and every guard byte must still be 0xEE."""
import numpy as np
import pytest

from resql_amd import plan as P

pytestmark = pytest.mark.gpu
T = P.TypeInit
TILE = 49152          # result_pack.hip PK_TILE_BYTES
GUARD = 64

SCHEMAS = {
    "int": [T.INT()],                                                                                    # 4 bytes a tuple
    "bool_int": [T.BOOL(), T.INT()],                                                                     # 5: spans start at every alignment
    "mixed": [T.CHAR(1), T.BIGINT(), T.VARCHAR(7), T.DATE(), T.DECIMAL(15, 2), T.CHAR(3)],               # 34
    "bools64": [T.BOOL()] * 64,                                                                          # 64 columns
    "varchar199": [T.VARCHAR(199), T.INT()],                                                             # 204: R = 240
    "varchar300": [T.VARCHAR(300), T.BIGINT()],                                                          # 309: R = 159
    "long": [T.VARCHAR(50000), T.INT()],                                                                 # 50005: longer than the tile
}
TUPLE_SIZE = {"int": 4, "bool_int": 5, "mixed": 34, "bools64": 64, "varchar199": 204, "varchar300": 309, "long": 50005}
GROUP_ROWS = {"int": 256, "bool_int": 256, "mixed": 256, "bools64": 256, "varchar199": 240, "varchar300": 159, "long": 0}


def is_string(t):
    return t.tag == P.VARCHAR or (t.tag == P.CHAR and t.len > 1)


def field_size(t):
    return t.width + 1 if t.tag in (P.CHAR, P.VARCHAR) else t.width          # (CHAR(1): its byte and a zero)


def cells_of(t, n, R, seed):
    """n cells of type t as uint8 [n, width]: every byte value in the numbers; strings of every length with non-zero bytes behind their
    NUL, and in the first and last row of each tile a full-width string without a NUL, an empty one, a NUL in front of non-zero bytes"""
    w = t.width
    junk = ((np.arange(n * w, dtype=np.uint64) * np.uint64(2654435761 + 2 * seed) >> np.uint64(11)) % np.uint64(256)).astype(np.uint8).reshape(n, w)
    if not is_string(t):
        return junk
    cells = junk | np.uint8(1)                                                                     # no NUL by accident
    lengths = (np.arange(n, dtype=np.int64) * 7 + seed) % (w + 1)
    for r in range(n):
        if lengths[r] < w:
            cells[r, lengths[r]] = 0                                                               # (what lies behind stays non-zero)
    step = R if R else 1
    special = sorted({r for r in (0, step - 1, step, 2 * step - 1, 2 * step, n - 1) if 0 <= r < n})
    for i, r in enumerate(special):
        kind = (i + seed) % 3
        cells[r] = junk[r] | np.uint8(1)                                                           # a full-width string without a NUL
        if kind == 1:
            cells[r] = 0                                                                           # an empty string
        elif kind == 2:
            cells[r, 0] = 0                                                                        # a NUL followed by non-zero bytes
    return cells


def restated(types, columns, n):
    """the tuples as uint8 [n, tuple size]: field c at the sum of the field sizes in front of it; a number's cell as it is; CHAR(1)'s byte,
    then 0; a string's bytes in front of its first NUL, 0 from there to the end of its width + 1 bytes"""
    ts = sum(field_size(t) for t in types)
    out = np.full((n, ts), 0xEE, dtype=np.uint8)
    off = 0
    for t, cells in zip(types, columns):
        fs = field_size(t)
        field = np.zeros((n, fs), dtype=np.uint8)
        if is_string(t):
            in_front = np.cumprod(cells != 0, axis=1).astype(bool)          # True up to, not including, the first NUL
            field[:, :t.width] = np.where(in_front, cells, 0)
        else:
            field[:, :t.width] = cells
        out[:, off:off + fs] = field
        off += fs
    assert off == ts
    return out


def row_counts(R):
    return [1, R - 1, R, R + 1, 2 * R + 1, 1000] if R else [3]


CASES = [(name, n) for name in SCHEMAS for n in row_counts(GROUP_ROWS[name])]


def test_the_schemas_are_the_ones_the_kernel_tiles_as_described():
    for name, types in SCHEMAS.items():
        ts = sum(field_size(t) for t in types)
        assert ts == TUPLE_SIZE[name] and GROUP_ROWS[name] == (min(256, TILE // ts) if ts <= TILE else 0), name


@pytest.mark.parametrize("name,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_every_byte_against_the_restatement(gpu_ctx, name, n):
    types = SCHEMAS[name]
    columns = [cells_of(t, n, GROUP_ROWS[name], seed=c) for c, t in enumerate(types)]
    want = restated(types, columns, n)
    got = gpu_ctx.prim_pack_tuples(columns, types)
    ts = TUPLE_SIZE[name]
    assert got.shape == (n * ts + GUARD,)
    tuples = got[:n * ts].reshape(n, ts)
    wrong = np.flatnonzero((tuples != want).any(axis=1))
    assert len(wrong) == 0, "rows %s differ; row %d: got %s want %s" % (wrong[:8], wrong[0], tuples[wrong[0]].tobytes()[:80], want[wrong[0]].tobytes()[:80])
    assert (got[n * ts:] == 0xEE).all(), "a byte behind the last tuple was written"


def test_the_restatement_spells_a_known_tuple():
    """the restatement itself, against bytes spelled out: CHAR(1) 'R', BIGINT, VARCHAR(7) "ab" with bytes behind its NUL, CHAR(3) full"""
    types = [T.CHAR(1), T.BIGINT(), T.VARCHAR(7), T.CHAR(3)]
    columns = [np.array([[ord("R")]], dtype=np.uint8), np.array([0x0102030405060708], dtype=np.int64).view(np.uint8).reshape(1, 8),
               np.frombuffer(b"ab\0xyz!", dtype=np.uint8).reshape(1, 7), np.frombuffer(b"abc", dtype=np.uint8).reshape(1, 3)]
    assert restated(types, columns, 1).tobytes() == b"R\0" + bytes([8, 7, 6, 5, 4, 3, 2, 1]) + b"ab\0\0\0\0\0\0" + b"abc\0"

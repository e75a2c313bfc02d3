"""Tables of a MultiContext's shards for the GPU tests: every shard holds a table whole (replicated) or a row slice of it with its first
row set.  Which rows a named cut gives each shard is the test file's own: it passes `cuts(table, kind, n_shards)` -> the n_shards + 1 row
boundaries."""
import numpy as np

from resql_amd import plan as P


def slice_rows(t: P.Table, lo: int, hi: int) -> P.Table:
    return P.Table(t.name, [P.Column(c.name, c.type, None if c.data is None else np.ascontiguousarray(c.data[lo:hi])) for c in t.columns], hi - lo)


class Shards:
    """per shard context: the whole table (cut None) or its slice under a named cut, made on first use"""

    def __init__(self, m, tables, cuts):
        self.m, self.tables, self.cuts, self.made = m, tables, cuts, {}

    def get(self, i, name, cut=None):
        key = (i, name, cut)
        if key not in self.made:
            t = self.tables[name]
            if cut is None:
                self.made[key] = self.m.shards[i].table(t)
            else:
                c = self.cuts(t, cut, self.m.n)
                d = self.m.shards[i].table(slice_rows(t, c[i], c[i + 1]))
                d.set_row0(c[i])
                self.made[key] = d
        return self.made[key]

    def layout(self, names, cut_of):
        return [[self.get(i, k, cut_of.get(k)) for k in names] for i in range(self.m.n)]

    def close(self):
        for t in self.made.values():
            t.close()

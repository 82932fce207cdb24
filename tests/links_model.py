"""A plain model of the PE-link table (K5, ``vs_links_*``): Python ints and numpy, nothing of the product.

``process_pe_info`` (the reference's VStrains_IO.py:598-627) reads the lines ``u:v:count`` of pe_info and of st_info and adds
every count under the key (min(u, v), max(u, v)).  For two n x n matrices of such counts the key {i, j}, i != j, therefore
holds node[i][j] + node[j][i] + short[i][j] + short[j][i], and the key {i, i} holds node[i][i] + short[i][i].  The table P0
answers P0[i][j] = P0[j][i] = key {i, j}.  Every later read of the stages is a block sum over P0: the sum of P0[r][c] over
a list of rows and a list of columns, an index counted as often as it occurs in its list.

The model keeps the keys in a dict of Python ints (no wrap-around, no n x n array unless ``dense`` is asked for), so it also
serves tables of thousands of nodes that hold a few thousand cells."""
import numpy as np


class LinksModel:
    def __init__(self, n, lines):
        """``lines``: (u, v, count) with 0 <= u, v < n, in any order, repeats allowed -- the lines of both files."""
        self.n = int(n)
        keys = {}
        for u, v, count in lines:
            u, v = int(u), int(v)
            assert 0 <= u < self.n and 0 <= v < self.n
            k = (u, v) if u <= v else (v, u)
            keys[k] = keys.get(k, 0) + int(count)
        self.keys = keys
        rows = {}
        for (u, v), s in keys.items():
            if s:
                rows.setdefault(u, {})[v] = s
                rows.setdefault(v, {})[u] = s
        self.rows = rows  # row -> {column: non-zero P0[row][column]}

    @classmethod
    def from_matrices(cls, node, short):
        """The lines a dense pe_info / st_info pair holds, one per cell of either matrix (a count of zero adds nothing)."""
        node, short = np.asarray(node), np.asarray(short)
        n = node.shape[0]
        assert node.shape == (n, n) and short.shape == (n, n)
        lines = []
        for mat in (node, short):
            vals = mat.tolist()
            for i in range(n):
                row = vals[i]
                lines.extend((i, j, row[j]) for j in range(n) if row[j])
        return cls(n, lines)

    @classmethod
    def from_cells(cls, n, rows, cols, vals):
        return cls(n, zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(vals).tolist()))

    def cell(self, r, c):
        return self.rows.get(r, {}).get(c, 0)

    def dense(self):
        """P0 as an n x n int64 array (small tables only); a value outside int64 is an error of the case."""
        out = np.zeros((self.n, self.n), dtype=np.int64)
        for r, d in self.rows.items():
            for c, s in d.items():
                out[r, c] = s
        return out

    def csr(self):
        """(row_ptr uint32 [n + 1], col uint32 [nnz], val int64 [nnz]): the non-zero cells of every row, columns strictly
        ascending."""
        row_ptr = np.zeros(self.n + 1, dtype=np.uint32)
        col, val = [], []
        for r in range(self.n):
            d = self.rows.get(r)
            if d:
                for c in sorted(d):
                    col.append(c)
                    val.append(d[c])
            row_ptr[r + 1] = len(col)
        return row_ptr, np.asarray(col, dtype=np.uint32), np.asarray(val, dtype=np.int64)

    def row_lengths(self):
        return [len(self.rows.get(r, ())) for r in range(self.n)]

    def block_sum(self, rows, cols):
        s = 0
        for r in rows:
            d = self.rows.get(r)
            if d:
                for c in cols:
                    s += d.get(c, 0)
        return s

    def block_sums(self, queries):
        return [self.block_sum(rows, cols) for rows, cols in queries]

    def group_matrix(self, groups):
        """Python ints, row g = [block_sum(groups[g], groups[h]) for every h]."""
        return [[self.block_sum(a, b) for b in groups] for a in groups]

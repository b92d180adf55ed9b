"""igraph stand-in for running the reference's `DVAE_PYG.decode()` (dvae/models_pyg.py:338-396) in
tests/golden/make_golden_dvae_decode.py.  Beyond what oracle/pyg_standin/igraph offers, `decode()` touches
`g.vs.select(_outdegree_eq=0)`, `v.index` and `del g.vs[name]`; the deleted attribute values are kept in
`g.vs.deleted[name]`, so that the generator can read the final states the reference throws away."""


class _Vertex(dict):
    def __init__(self, graph, index, attrs):
        dict.__init__(self, attrs)
        self._graph, self.index = graph, index


class _VertexSeq(list):
    def __init__(self):
        list.__init__(self)
        self.deleted = {}

    def __setitem__(self, key, value):
        if isinstance(key, str):
            for vtx, val in zip(self, value):
                vtx[key] = val
        else:
            list.__setitem__(self, key, value)

    def __getitem__(self, key):
        if isinstance(key, str):
            return [vtx.get(key) for vtx in self]
        return list.__getitem__(self, key)

    def __delitem__(self, key):
        if not isinstance(key, str):
            raise NotImplementedError("igraph stand-in: only attributes can be deleted")
        self.deleted[key] = [vtx.pop(key, None) for vtx in self]

    def select(self, _outdegree_eq=None, **kw):
        if kw or _outdegree_eq is None:
            raise NotImplementedError("igraph stand-in: select(_outdegree_eq=k) only")
        return [v for v in self if v._graph.outdegree(v.index) == _outdegree_eq]


class Graph:
    def __init__(self, directed=True, **_):
        if not directed:
            raise NotImplementedError("igraph stand-in: directed graphs only")
        self.vs = _VertexSeq()
        self._edges = []

    def add_vertices(self, n):
        for _ in range(n):
            self.add_vertex()

    def add_vertex(self, **attrs):
        self.vs.append(_Vertex(self, len(self.vs), attrs))

    def add_edge(self, u, v):
        self._edges.append((int(u), int(v)))

    def add_edges(self, edges):
        for u, v in edges:
            self.add_edge(u, v)

    def vcount(self):
        return len(self.vs)

    def ecount(self):
        return len(self._edges)

    def get_edgelist(self):
        return list(self._edges)

    def predecessors(self, v):
        return sorted(u for u, w in self._edges if w == v)

    def successors(self, v):
        return sorted(w for u, w in self._edges if u == v)

    def outdegree(self, v):
        return sum(1 for u, _ in self._edges if u == v)

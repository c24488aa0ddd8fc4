"""The few pieces of DGL that the reference's PCM uses, for the golden generator only (oracle/make_golden.py).

Written from DGL's documented semantics: a graph is an edge list (edge ids in insertion order) plus a node-feature
dict `ndata`; `update_all(message_func, reduce_func)` computes one message per edge from the source node's features,
groups the destination nodes by in-degree ("degree bucketing"), hands each bucket a mailbox [n_nodes, degree, ...]
whose second axis runs over a node's incoming edges in edge-id order, and writes the reduced values back into
`ndata`.  Only what PCM.init_graph / PCM.forward touch is provided:

    dgl.DGLGraph(nx_digraph), graph.ndata, graph.to(device), graph.update_all(message_func, reduce_func),
    dgl.transform.remove_self_loop(graph)

Nodes without incoming edges are not reduced (their output rows stay zero).  Everything is plain torch and
differentiable: the results are scattered into `ndata` out of place, so autograd reaches the node features and the
parameters used inside message_func / reduce_func.  The product never imports this module.
"""
import types

import torch


class _Batch:
    def __init__(self, **fields):
        self.__dict__.update(fields)


class DGLGraph:
    def __init__(self, graph=None, src=None, dst=None, num_nodes=None):
        if graph is not None:           # networkx (Di)Graph: nodes 0..N-1, edges in the graph's own iteration order
            num_nodes = graph.number_of_nodes()
            pairs = list(graph.edges())
            src = [int(u) for u, _ in pairs]
            dst = [int(v) for _, v in pairs]
        self.src = torch.as_tensor(src, dtype=torch.int64)
        self.dst = torch.as_tensor(dst, dtype=torch.int64)
        self._n = int(num_nodes)
        self.ndata = {}

    def number_of_nodes(self):
        return self._n

    def number_of_edges(self):
        return int(self.src.numel())

    def edges(self):
        return self.src, self.dst

    def to(self, device):
        return self

    def update_all(self, message_func, reduce_func):
        E = self.number_of_edges()
        msgs = message_func(_Batch(src={k: v[self.src] for k, v in self.ndata.items()},
                                   dst={k: v[self.dst] for k, v in self.ndata.items()}, data={}))
        # a stable sort by destination keeps each node's incoming edges in edge-id order
        order = torch.sort(self.dst, stable=True).indices
        dst_sorted = self.dst[order]
        nodes, deg = torch.unique_consecutive(dst_sorted, return_counts=True)
        first = torch.cumsum(deg, 0) - deg                  # position of each node's first edge in `order`
        out = {}
        for d in torch.unique(deg).tolist():                # one reduce_func call per degree bucket
            sel = (deg == d).nonzero().flatten()
            bucket = nodes[sel]
            eids = order[first[sel][:, None] + torch.arange(d)[None, :]]        # [n_nodes, d]
            mailbox = {k: m[eids] for k, m in msgs.items()}
            res = reduce_func(_Batch(mailbox=mailbox, data={k: v[bucket] for k, v in self.ndata.items()}, nodes=bucket))
            for k, v in res.items():
                base = out[k] if k in out else v.new_zeros((self._n,) + tuple(v.shape[1:]))
                out[k] = base.index_copy(0, bucket, v)
        assert E == 0 or int(deg.sum()) == E
        self.ndata.update(out)


def _remove_self_loop(g):
    keep = g.src != g.dst
    return DGLGraph(src=g.src[keep], dst=g.dst[keep], num_nodes=g.number_of_nodes())


transform = types.SimpleNamespace(remove_self_loop=_remove_self_loop)

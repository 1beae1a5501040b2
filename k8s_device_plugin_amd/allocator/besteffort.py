"""Best-effort topology-aware preferred allocation.

Semantics match the reference policy (reference:
internal/pkg/allocator/besteffort_policy.go:88-151, device.go:255-443):

  - fast paths: available==size -> available; required==size -> required;
  - partitions are grouped by physical GPU (devID); groups are sorted
    ascending by free-partition count (tie: parent id) so nearly-full GPUs
    are packed first (anti-fragmentation);
  - candidate sets are seeded per group (prefer one whole GPU's partitions)
    and breadth-first extended across groups when one GPU cannot satisfy
    the request;
  - the candidate with the minimum total pairwise weight wins.

There is one search (_search) with two scorers: per group in closed form
when every partition pair of the same two GPUs weighs the same, per node
otherwise.  native/pref_alloc.h is the same search in C++ for the native
server; the differential tests hold the two to identical id lists.

The pair weights themselves are hive-aware (weights.py), which on an
8*MI355X node packs 2/4/8-GPU requests onto one xGMI hive.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

from ..topology.discovery import GPUDevice
from ..topology.kfd import KFDTopology
from ..topology.sysfs import SysPaths
from .weights import compute_pair_weights


class AllocationError(ValueError):
    pass


@dataclass
class _Group:
    """Free partitions of one physical GPU available to this request."""

    dev_id: str
    parent_id: str
    node_ids: List[int]  # ascending


class BestEffortPolicy:
    """Preferred-allocation policy; init once at plugin start, then allocate
    from memory with zero I/O (reference: plugin.go:85)."""

    def __init__(self) -> None:
        self._devices: Dict[str, GPUDevice] = {}
        self._weights: Dict[int, Dict[int, int]] = {}
        self._groups: Dict[str, _Group] = {}
        self._initialized = False
        self._uniform = False
        self._gw: Dict[str, Dict[str, int]] = {}
        self._group_of_node: Dict[int, str] = {}

    def init(
        self,
        devices: Iterable[GPUDevice],
        topology: Optional[KFDTopology] = None,
        paths: SysPaths = SysPaths(),
    ) -> None:
        devs = list(devices)
        if not devs:
            raise AllocationError("no devices to initialize allocator with")
        topo = topology if topology is not None else KFDTopology.load(paths)
        self._weights = compute_pair_weights(devs, topo)
        if not self._weights and len(devs) > 1:
            # Multiple devices but zero GPU-GPU links in the topology: the
            # reference's Init fails here and the plugin silently drops
            # GetPreferredAllocation (besteffort_policy.go:70-86,
            # plugin.go:86-89).  We instead degrade to a zero-weight table:
            # candidates are then ranked purely by the anti-fragmentation
            # group ordering, which is still deterministic and correct —
            # and the preferred-allocation path stays advertised (and
            # measurable) instead of vanishing.
            import logging

            logging.getLogger(__name__).warning(
                "no inter-device links in topology for %d devices; serving "
                "preferred allocation with uniform weights", len(devs)
            )
        self._devices = {d.id: d for d in devs}
        self._groups = {}
        for d in devs:
            g = self._groups.setdefault(d.dev_id, _Group(d.dev_id, "", []))
            g.node_ids.append(d.node_id)
            if not d.is_partition:
                g.parent_id = d.id
        for g in self._groups.values():
            g.node_ids.sort()
        self._build_uniform_table()
        self._initialized = True

    def _build_uniform_table(self) -> None:
        """Group-pair weight table when the topology is uniform.

        The weight model derives a pair's score from per-GPU facts (same
        devID, link type, NUMA, hive — weights.py), so every partition
        pair of the same two physical GPUs normally scores identically.
        When that holds for the loaded topology (verified here, never
        assumed), allocate() scores with _uniform_scorer, else with
        _per_node_scorer; the totals, and so the results, are identical.
        Same check as AllocState::build_uniform_table in
        native/pref_alloc.h.
        """
        self._uniform = True
        self._gw: Dict[str, Dict[str, int]] = {}
        self._group_of_node: Dict[int, str] = {}
        keys = list(self._groups)
        for k in keys:
            for n in self._groups[k].node_ids:
                self._group_of_node[n] = k

        def w(a: int, b: int) -> int:
            if a > b:
                a, b = b, a
            return self._weights.get(a, {}).get(b, 0)

        for i, ka in enumerate(keys):
            ga = self._groups[ka].node_ids
            for kb in keys[i:]:
                gb = self._groups[kb].node_ids
                first = True
                w0 = 0
                for x in ga:
                    for y in gb:
                        if ka == kb and x >= y:
                            continue
                        wxy = w(x, y)
                        if first:
                            w0, first = wxy, False
                        elif wxy != w0:
                            self._uniform = False
                            return
                self._gw.setdefault(ka, {})[kb] = w0
                self._gw.setdefault(kb, {})[ka] = w0

    @property
    def initialized(self) -> bool:
        return self._initialized

    def export_state(self):
        """State for the native fast server's in-C++ search: (groups as
        [(parent_id, sorted node_ids)], {device_id: node_id},
        [(node_a, node_b, weight)])."""
        groups = [(g.parent_id, sorted(g.node_ids)) for g in self._groups.values()]
        node_of_id = {d.id: d.node_id for d in self._devices.values()}
        weights = [
            (a, b, w) for a, inner in self._weights.items() for b, w in inner.items()
        ]
        return groups, node_of_id, weights

    def allocate(
        self,
        available_ids: Sequence[str],
        required_ids: Sequence[str],
        size: int,
    ) -> List[str]:
        if size <= 0:
            raise AllocationError("allocation size must be a positive integer")
        if len(available_ids) < size:
            raise AllocationError("available devices count less than allocation size")
        if len(required_ids) > size:
            raise AllocationError("must-include set larger than allocation size")
        if len(required_ids) > len(available_ids):
            raise AllocationError("must-include set larger than available set")
        if not self._devices:
            raise AllocationError("allocator not initialized")
        if len(available_ids) == size:
            return list(available_ids)
        if len(required_ids) == size:
            return list(required_ids)
        if not set(required_ids).issubset(set(available_ids)):
            raise AllocationError("must-include devices not all available")

        available = [self._devices[i] for i in available_ids if i in self._devices]
        required = [self._devices[i] for i in required_ids if i in self._devices]
        groups = self._filtered_groups(available, required)
        req_nodes = [d.node_id for d in required]
        make_scorer = self._uniform_scorer if self._uniform else self._per_node_scorer
        nodes = _search(groups, size - len(required), req_nodes,
                        make_scorer(groups, req_nodes))
        by_node = {d.node_id: d.id for d in available}
        return [by_node[n] for n in nodes if n in by_node]

    # ---- internals ----

    def _filtered_groups(
        self, available: Sequence[GPUDevice], required: Sequence[GPUDevice]
    ) -> List[_Group]:
        avail_ids = {d.node_id for d in available}
        req_ids = {d.node_id for d in required}
        groups: List[_Group] = []
        for g in self._groups.values():
            ids = sorted(i for i in g.node_ids if i in avail_ids and i not in req_ids)
            if ids:
                groups.append(_Group(g.dev_id, g.parent_id, ids))
        groups.sort(key=lambda g: (len(g.node_ids), g.parent_id))
        return groups

    # A scorer is (extra of the empty state, add, finish): add(st, fidx, m)
    # gives (weight, extra) of st plus the first m nodes of filtered group
    # fidx; finish(st) gives a complete state's weight with the required
    # nodes added.

    def _uniform_scorer(self, groups, req_nodes):
        """Closed form under verified-uniform group-pair weights: with
        rowsum[b] = sum_h count[h]*gw[b][h] carried as the state's extra,
        adding m nodes of group b costs m*rowsum[b] + C(m,2)*gw[b][b] —
        O(G) per group instead of O(|subset|) per node, same totals."""
        gkeys = [g.dev_id for g in groups]
        gw = self._gw
        group_of_node = self._group_of_node

        def add_row(rowsum, b, m):
            rowsum = dict(rowsum)
            for h, wbh in gw[b].items():
                rowsum[h] = rowsum.get(h, 0) + m * wbh
            return rowsum

        def add(st, fidx, m):
            b = gkeys[fidx]
            rowsum = st[4]
            weight = st[3] + m * rowsum.get(b, 0) + m * (m - 1) // 2 * gw[b][b]
            return weight, add_row(rowsum, b, m)

        def finish(st):
            weight, rowsum = st[3], st[4]
            for rn in req_nodes:
                b = group_of_node[rn]
                weight += rowsum.get(b, 0)
                rowsum = add_row(rowsum, b, 1)
            return weight

        return {}, add, finish

    def _per_node_scorer(self, groups, req_nodes):
        """Exact for any weight table: each new node is scored against
        every node already in the state and the earlier new ones."""
        weights = self._weights

        def score(st, new_nodes):
            nodes = _state_nodes(groups, st[1], st[2])
            w = st[3]
            for n in new_nodes:
                for o in nodes:
                    frm, to = (o, n) if o < n else (n, o)
                    w += weights.get(frm, {}).get(to, 0)
                nodes.append(n)
            return w

        return (None,
                lambda st, fidx, m: (score(st, groups[fidx].node_ids[:m]), None),
                lambda st: score(st, req_nodes))


def _state_nodes(groups: List[_Group], order, size: int) -> List[int]:
    """A state's nodes: its groups in add order, the last one as a prefix."""
    nodes: List[int] = []
    for fidx in order:
        nodes.extend(groups[fidx].node_ids[:size - len(nodes)])
    return nodes


def _search(groups: List[_Group], new_size: int, req_nodes: List[int],
            scorer) -> List[int]:
    """Seed one state per group, extend breadth-first across groups for
    requests no single GPU can satisfy (reference: device.go:406-441) and
    return the nodes of the first strict-minimum complete state in
    generation order, required nodes last.

    A state is (parent bitset, group add order, size, weight, scorer's
    extra).  An incomplete state holds ALL free nodes of every group it
    added, so it is fully determined by the parent SET; the reference
    re-expands every parent-order permutation (O(G!) states), we dedupe on
    the set (O(2^G)), which makes 64-partition CPX requests tractable
    without changing any result.
    """
    empty, add, finish = scorer
    n_groups = len(groups)
    best = None  # (weight, order)
    queue: list = []
    seen = set()

    def extend(st, idx):
        nonlocal best
        take = min(len(groups[idx].node_ids), new_size - st[2])
        weight, extra = add(st, idx, take)
        st = (st[0] | (1 << idx), st[1] + (idx,), st[2] + take, weight, extra)
        if st[2] == new_size:
            w = finish(st)
            if best is None or w < best[0]:
                best = (w, st[1])
        elif st[0] not in seen:
            seen.add(st[0])
            queue.append(st)

    for idx in range(n_groups):
        extend((0, (), 0, 0, empty), idx)
    for cur in queue:  # grows while it is walked
        if bin(cur[0]).count("1") == n_groups:
            continue
        for idx in range(n_groups):
            if not cur[0] & (1 << idx):
                extend(cur, idx)
    if best is None:
        raise AllocationError("no candidate subset found with matching criteria")
    return _state_nodes(groups, best[1], new_size) + req_nodes

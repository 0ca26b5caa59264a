"""An independent model of lrm_pose_routes_* (include/lrm.h) in pure Python: heapq Dijkstra on (cost, hops) tuples of
unbounded Python ints with the cap applied, predecessors chosen by the definition in a loop over the edges.  It shares
nothing with the C code: no packed key, no counting sort, no ctypes."""
import heapq

CAP = 4294967294  # the largest sum of costs a route may have


def arcs_of(nposes, edge_a, edge_b, edge_live=None, pose_live=None, edge_cost=None, direction=0):
    """[(e, u, v, w)] in ascending e: the arcs u -> v of the usable edges"""
    def pose_ok(p):
        return 0 <= p < nposes and (pose_live is None or pose_live[p] != 0)

    out = []
    for e, (a, b) in enumerate(zip(edge_a, edge_b)):
        a, b = int(a), int(b)
        w = 1 if edge_cost is None else int(edge_cost[e])
        if (edge_live is not None and edge_live[e] == 0) or not pose_ok(a) or not pose_ok(b) or w < 0:
            continue
        if direction in (0, 1):
            out.append((e, a, b, w))
        if direction in (0, 2):
            out.append((e, b, a, w))
    return out


def routes(nposes, edge_a, edge_b, sources, edge_live=None, pose_live=None, edge_cost=None, direction=0):
    """-> dict(cost, hops, pred_edge, pred_pose: lists of nposes ints; reached; tight: tight incoming arcs per pose)"""
    arcs = arcs_of(nposes, edge_a, edge_b, edge_live, pose_live, edge_cost, direction)
    out_of = [[] for _ in range(nposes)]
    for e, u, v, w in arcs:
        out_of[u].append((v, w))
    key = [None] * nposes
    heap = []
    for s in sources:
        s = int(s)
        if 0 <= s < nposes and (pose_live is None or pose_live[s] != 0) and key[s] is None:
            key[s] = (0, 0)
            heap.append(((0, 0), s))
    heapq.heapify(heap)
    while heap:
        k, u = heapq.heappop(heap)
        if k != key[u]:
            continue
        for v, w in out_of[u]:
            c = (k[0] + w, k[1] + 1)
            if c[0] <= CAP and (key[v] is None or c < key[v]):
                key[v] = c
                heapq.heappush(heap, (c, v))
    pred_edge, pred_pose, tight = [-1] * nposes, [-1] * nposes, [0] * nposes
    for e, u, v, w in arcs:  # ascending e: the first tight arc into v is the smallest edge's
        if key[u] is None or key[v] is None or (key[u][0] + w, key[u][1] + 1) != key[v]:
            continue
        tight[v] += 1
        if pred_edge[v] < 0:
            pred_edge[v], pred_pose[v] = e, u
    return {"cost": [-1 if k is None else k[0] for k in key], "hops": [-1 if k is None else k[1] for k in key],
            "pred_edge": pred_edge, "pred_pose": pred_pose, "reached": sum(k is not None for k in key), "tight": tight}

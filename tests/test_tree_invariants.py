"""The tree a commit stages for upload, read back on the CPU (rs_probe_tree through DeviceScene.tree(), host-only
commits: no GPU). The f32 cull of the walks (raysnail_amd/csrc/rs_cull.h) may only ever be conservative if every
leaf's exact f64 box lies inside every f32 box above it, and the walks' stacks and orders rest on the tree's shape:

  structure     node 0 is the root, every other node and every leaf entry is referenced exactly once, the leaves are a
                permutation of the world's prims, empty slots hold INT32_MIN with planes (+inf, -inf), and in the
                in-order tree they come only after the filled ones (walk4_inorder ends a node at the first);
  containment   every slot's f32 box, widened exactly to f64, holds the pbox of every prim below it (an infinite
                bound needs an infinite plane; none of these scenes has a NaN bound, which is asserted);
  pbox          equals the oracle's bounding_box of the same handle over the scene's time range, bit for bit (a zero
                bound may carry either sign: test_pbox_is_the_oracles_bounding_box says why);
  stack_need    and tree_depth equal a recomputation from the exported tree by the rules above rs_host.cpp's
                stack_needW / stack_need4_ref / stack_need2 / stack_need_ref, and walks of each kind with every box
                test passing never hold more entries (one order of each reaches the bound);
  tree top      in spheres mode the first ltop nodes are the breadth-first top;
  leaf order    in reference-order scenes the in-order leaf sequence is the oracle's BVH's, left to right."""
import functools

import numpy as np
import pytest

import edge_rays as E
import far_worlds as F
from raysnail_amd import scenes
from raysnail_amd.api import DeviceScene

EMPTY = -2 ** 31
VARIANTS = ("plain", "t29", "s-100", "s100")
SCENES = [f"{n}:{v}" for n in F.NAMES for v in VARIANTS] + ["quadric_sdl", "mesh", "deep_spheres", "skewed"]


@functools.lru_cache(maxsize=None)
def _world(key: str):
    if ":" in key:
        name, variant = key.split(":")
        return E.world(name) if variant == "plain" else F.world(name, variant)
    if key == "quadric_sdl":
        return scenes.quadric_sdl(32, 32)[1]
    if key == "mesh":
        return scenes.mesh_scene(48, 27, 14, 30)[1]
    if key == "deep_spheres":
        return scenes.deep_spheres(80, 50, 2000)[1]
    from test_tree_build import skewed_world
    return skewed_world()


@functools.lru_cache(maxsize=None)
def _scene(key: str):
    ds = DeviceScene(_world(key), devices=[])
    return ds, ds.tree(), ds.info()


@functools.lru_cache(maxsize=None)
def _oracle(key: str):
    from oracle.binding import OracleScene
    return OracleScene(_world(key))


def _prim(t, code: int) -> int:
    e = ~code
    return int(t["lprim"][e]) if len(t["lprim"]) else e


def _inner_nodes_postorder(t):
    """Node indices, children before parents (iterative: the skewed tree is deep)."""
    order, stack = [], [t["root"]]
    while stack:
        n = stack.pop()
        order.append(n)
        stack.extend(int(c) for c in t["child"][n] if c >= 0)
    return order[::-1]


@pytest.mark.parametrize("key", SCENES)
def test_structure(key):
    ds, t, info = _scene(key)
    child, planes = t["child"], t["planes"]
    n_nodes, arity = child.shape
    assert arity == info.tree_arity and n_nodes == info.n_nodes and t["ref_order"] == info.ref_order
    assert t["root"] == 0
    refs = np.bincount(child[child >= 0], minlength=n_nodes)
    assert refs[0] == 0 and (refs[1:] == 1).all()
    assert len(_inner_nodes_postorder(t)) == n_nodes                     # and all of them below the root
    leaves = child[(child < 0) & (child != EMPTY)]
    entries = np.sort(~leaves)
    world = np.sort(_oracle(key).leaf_order().astype(np.int64))          # the world's handles
    assert len(world) == info.n_world
    if len(t["lprim"]):
        assert np.array_equal(entries, np.arange(len(t["lprim"])))       # every leaf entry exactly once
        assert np.array_equal(np.sort(t["lprim"]), world)                # a permutation of the world's prims
    else:
        assert np.array_equal(entries, world)
    empty = child == EMPTY
    inf = np.float32(np.inf)
    assert (planes[empty][:, :3] == inf).all() and (planes[empty][:, 3:] == -inf).all()
    # a filled slot is a box: lo <= hi on every axis
    assert (planes[~empty][:, :3] <= planes[~empty][:, 3:]).all()
    assert not empty[:, 0].any()                                         # no node without a first child
    if t["ref_order"] and arity == 4:
        assert not (empty[:, :-1] & ~empty[:, 1:]).any()                 # empty slots only after the filled ones


@pytest.mark.parametrize("key", SCENES)
def test_containment(key):
    ds, t, info = _scene(key)
    child, pbox = t["child"], t["pbox"]
    planes = t["planes"].astype(np.float64)                              # exact
    assert not np.isnan(pbox).any() and not np.isnan(planes).any()
    n_nodes, arity = child.shape
    lo = np.full((n_nodes, 3), np.inf)
    hi = np.full((n_nodes, 3), -np.inf)
    checked = 0
    for n in _inner_nodes_postorder(t):
        for k in range(arity):
            c = int(child[n, k])
            if c == EMPTY:
                continue
            if c < 0:
                b = pbox[_prim(t, c)]
                slo, shi = b[:3], b[3:]
            else:
                slo, shi = lo[c], hi[c]
            # the slot's box holds everything below it (an infinite bound below needs an infinite plane: <= does it)
            assert (planes[n, k, :3] <= slo).all() and (planes[n, k, 3:] >= shi).all(), (key, n, k, planes[n, k], slo, shi)
            lo[n] = np.minimum(lo[n], slo)
            hi[n] = np.maximum(hi[n], shi)
            checked += 1
    assert checked == n_nodes - 1 + info.n_world


@pytest.mark.parametrize("key", SCENES)
def test_pbox_is_the_oracles_bounding_box(key):
    """Every handle, nested children included: sphere and moving sphere, the three rects, triangle, box, quadric,
    Intersection and Difference, translated / rotated / scaled TfFacades, ConstantMedium (the kinds are counted
    over all scenes in test_kinds_covered)."""
    ds, t, info = _scene(key)
    orc = _oracle(key)
    pbox = t["pbox"]
    assert len(pbox) == info.n_objects
    handles = range(len(pbox)) if len(pbox) <= 3000 else range(0, len(pbox), 7)
    for h in handles:
        ref = orc.bbox(h)
        # bit for bit, but for the sign of a zero bound: a triangle's box is f64::max / min over its vertices
        # (vec3.rs:32-48), which leave the sign of max(+0, -0) open, as C's fmax / fmin do -- the host's compiler and
        # the oracle's choose differently, and no comparison slab64 makes tells the two zeros apart
        same = (E.bits(pbox[h]) == E.bits(ref)) | ((pbox[h] == 0.0) & (ref == 0.0))
        assert same.all(), (key, h, pbox[h], ref)


def test_kinds_covered():
    from raysnail_amd import api
    seen = set()

    def visit(o):
        seen.add(type(o).__name__ + (":moving" if isinstance(o, api.Sphere) and o.speed != (0.0, 0.0, 0.0) else "")
                 + (f":{o.plane}" if isinstance(o, api.AARect) else ""))
        for attr in ("o1", "o2", "plus", "minus", "boundary", "obj"):
            if hasattr(o, attr):
                visit(getattr(o, attr))
        if isinstance(o, api.TfFacade):
            for tf in o.stack.stack:
                seen.add(f"tf:{tf.kind}")
    for key in SCENES:
        for o in _world(key).hittables.objects:
            visit(o)
    from raysnail_amd import _abi as A
    want = {"Sphere", "Sphere:moving", "AARect:0", "AARect:1", "AARect:2", "TriangleMesh", "Box", "Quadric",
            "Intersection", "Difference", "TfFacade", "ConstantMedium", f"tf:{A.RS_TF_TRANSLATE}",
            f"tf:{A.RS_TF_ROTATE_Z}", f"tf:{A.RS_TF_SCALE}"}
    assert want <= seen, want - seen


# ---- stack_need and tree_depth, by the rules above rs_host.cpp's stack_need* ----
def _need(t, rule):
    """Bottom-up over the exported tree; rule(inner children's needs by slot, arity) -> the node's need."""
    child = t["child"]
    need = np.zeros(len(child), np.int64)
    for n in _inner_nodes_postorder(t):
        need[n] = rule([(k, int(need[c])) for k, c in enumerate(child[n]) if c >= 0], child.shape[1])
    return int(need[t["root"]])


def _rule_near4(inner, arity):       # a node pushes (inner children) - 1 entries, then the deepest child
    return max(len(inner) - 1, 0) + max([d for _, d in inner], default=0)


def _rule_ref4(inner, arity):        # the node (with its next slot) while an inner child before the last slot is searched
    return max([(1 if k < arity - 1 else 0) + d for k, d in inner], default=0)


def _rule_near2(inner, arity):       # one entry (the farther child) when both children are inner nodes
    return (1 if len(inner) == 2 else 0) + max([d for _, d in inner], default=0)


def _rule_ref2(inner, arity):        # the node itself while its left (inner) subtree is searched
    return max([(1 if k == 0 else 0) + d for k, d in inner], default=0)


def _expected_need(t):
    if t["arity"] == 4:
        return _need(t, _rule_ref4 if t["ref_order"] else _rule_near4)
    return _need(t, _rule_ref2) if t["ref_order"] else max(_need(t, _rule_ref2), _need(t, _rule_near2))


def _depth(t):
    depth = np.zeros(len(t["child"]), np.int64)
    for n in _inner_nodes_postorder(t):
        depth[n] = 1 + max([int(depth[c]) for c in t["child"][n] if c >= 0], default=0)
    return int(depth[t["root"]])


def _walk_max(t, pick):
    """The most entries a walk of the tree's kind holds when every box test passes. pick(inner children) orders a
    near-first node's inner children: the last is entered, the others are pushed."""
    child, arity = t["child"], t["arity"]
    most, sp = 0, 0
    if arity == 4 and not t["ref_order"]:
        stack, node = [], t["root"]
        while node is not None:
            inner = pick([int(c) for c in child[node] if c >= 0])
            if inner:
                stack.extend(inner[:-1])
                node = inner[-1]
            else:
                node = stack.pop() if stack else None
            most = max(most, len(stack))
        return most
    # reference order: slots left to right; entering an inner child before the last slot pushes the node
    stack, node, k = [], t["root"], 0
    while True:
        c = int(child[node, k]) if k < arity else EMPTY
        if k < arity and c != EMPTY:
            if c >= 0:
                if k < arity - 1:
                    stack.append((node, k + 1))
                    most = max(most, len(stack))
                node, k = c, 0
                continue
            k += 1
            continue
        if not stack:
            return most
        node, k = stack.pop()


@pytest.mark.parametrize("key", SCENES)
def test_stack_need_and_depth(key):
    ds, t, info = _scene(key)
    need = _expected_need(t)
    assert t["stack_need"] == info.stack_need == need, (key, t["stack_need"], info.stack_need, need)
    assert info.tree_depth == _depth(t)
    if t["arity"] == 4 and not t["ref_order"]:
        needs = {}
        child = t["child"]
        for n in _inner_nodes_postorder(t):
            needs[n] = _rule_near4([(k, needs[int(c)]) for k, c in enumerate(child[n]) if c >= 0], 4)
        orders = {"slot order": lambda inner: inner, "reversed": lambda inner: inner[::-1],
                  "deepest last": lambda inner: sorted(inner, key=lambda c: needs[c])}
        got = {name: _walk_max(t, pick) for name, pick in orders.items()}
        assert max(got.values()) <= need and got["deepest last"] == need, (key, got, need)
    else:
        got = _walk_max(t, None)
        if t["arity"] == 4 or t["ref_order"]:
            assert got == need, (key, got, need)
        else:
            assert got <= need, (key, got, need)


@pytest.mark.parametrize("key", [k for k in SCENES if k.startswith("spheres") or k in ("deep_spheres", "skewed")])
def test_tree_top_is_breadth_first(key):
    ds, t, info = _scene(key)
    assert info.scene_mode == 1
    ltop, child = t["ltop"], t["child"]
    assert 1 <= ltop == min(len(child), 85)
    parent = np.full(len(child), -1)
    depth = np.zeros(len(child), np.int64)
    for n in _inner_nodes_postorder(t)[::-1]:                            # parents before children
        for c in child[n]:
            if c >= 0:
                parent[c], depth[c] = n, depth[n] + 1
    top = np.arange(1, ltop)
    assert (parent[top] < top).all() and (parent[top] >= 0).all()
    assert (np.diff(depth[:ltop]) >= 0).all()
    if ltop < len(child):   # nothing shallower is left outside the top
        assert depth[ltop:].min() >= depth[ltop - 1]


@pytest.mark.parametrize("key", [k for k in SCENES if k.split(":")[0] in ("nest0", "nest2", "rich", "quadric_sdl")])
def test_reference_order_leaf_sequence(key):
    ds, t, info = _scene(key)
    assert t["ref_order"] == 1
    seq, stack = [], [t["root"]]
    while stack:
        c = stack.pop()
        if c >= 0:
            stack.extend(int(x) for x in t["child"][c][::-1] if x != EMPTY)
        else:
            seq.append(_prim(t, c))
    assert seq == [int(h) for h in _oracle(key).leaf_order()]


def test_other_scenes_are_not_reference_order():
    for key in SCENES:
        if key.split(":")[0] not in ("nest0", "nest2", "rich", "quadric_sdl"):
            assert _scene(key)[1]["ref_order"] == 0, key

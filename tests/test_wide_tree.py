"""Audit of the 4-wide culling tree the host collapse makes (csrc/host/wide_tree.hpp), on the CPU.

tests/wide_tree_host_check.cpp runs build_wide_tree -- the function plan_wide calls at upload -- under AddressSanitizer and
UndefinedBehaviorSanitizer and hands the records back; `audit` below judges them in numpy from the DEFINITION of the tree
(the comment at the head of wide_tree.hpp), not from its code:

  cut        the occupied children of wide node i are a cut of binary subtree i, one to three levels down: their leaves
             partition i's leaves
  order      they are the children "open the inner child of the largest half area until four slots are used" gives, in the
             same slots: an opened child is replaced by its first child, its second goes to the first free slot; ties go to
             the lowest slot, an area of 0 opens, a NaN area never does
  planes     a child's six planes are bit for bit the FlatNode32 planes of that child in its binary parent -- themselves the
             f64 planes rounded outward, restated here -- and enclose the f64 box
  empty      an empty slot holds code 0x7fffffff, lo = +inf, hi = -inf; every pad word is 0
  unreached  a binary node no wide walk reaches has an all-zero record
  levels     the highest stack slot any step can write, whichever children a ray hits and in whatever order, found by a
             recursion over the wide records that follows the step functions' stores (walk_node_step4, trace_vote.inc): with
             LdsStackB (slot 0 = "done", n starts at 1) it is levels - 1 exactly -- one level less overruns into the next LDS
             region, one more costs a resident block at 256 threads x 4 B -- and with LdsStack (n starts at 0) one lower.

The self-test corrupts copies of audited records and expects the matching failure, by name."""
import numpy as np
import pytest

import wide_tree_cases as wt

EMPTY = wt.EMPTY


class AuditError(AssertionError):
    def __init__(self, kind, msg):
        super().__init__("%s: %s" % (kind, msg))
        self.kind = kind


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _half_area(lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]


def expected_slots(nodes, i):
    """The definition, for binary node i: a list of (parent, side) positions, slot by slot."""
    slots = [(i, 0), (i, 1)]
    while len(slots) < 4:
        best, best_area = None, None
        for k, (p, c) in enumerate(slots):
            if nodes["child"][p, c] < 0:
                continue
            area = float(_half_area(nodes["bmin"][p, c], nodes["bmax"][p, c]))
            if area != area:
                continue  # NaN: never opens
            assert area >= 0.0, "the definition says nothing about a negative area (node %d side %d)" % (p, c)
            if best is None or area > best_area:  # strictly: a tie stays with the lower slot
                best, best_area = k, area
        if best is None:
            break
        n = int(nodes["child"][slots[best]])
        slots[best] = (n, 0)
        slots.append((n, 1))
    return slots


def _leaf_spans(nodes, root):
    """span[(p, c)] = (first, one past the last) leaf of child c of node p in depth-first order, for every position below root."""
    span, start, count = {}, {}, 0
    todo = [(root, 1), (root, 0)]
    while todo:
        item = todo.pop()
        if item[0] == "close":
            span[item[1]] = (start[item[1]], count)
            continue
        ch = int(nodes["child"][item])
        if ch < 0:
            span[item] = (count, count + 1)
            count += 1
        else:
            assert item not in start, "node %d is reached twice: not a tree" % ch
            start[item] = count
            todo += [("close", item), (ch, 1), (ch, 0)]
    return span


def stack_peaks(wide, root):
    """Highest slot written by a walk from `root`, RELATIVE to the n it starts with, for both stack types.

    One step at wide node i with n entries on the stack, nh of its children hit (any subset, any order):
      LdsStackB  four unconditional stores into slots n + nh - 1 - rank (hits) and n + nh - 1 (the nearest and the misses);
                 nh = 0 stores into n - 1.  Afterwards n' = n + nh - 1 and the nearest hit is the item; any of the other hits
                 is popped later with fewer entries below it.
      LdsStack   stores the nh hits into slots n .. n + nh - 1, pops the nearest: n' = n + nh - 1 as well.
    So a child is entered with n + j entries for any j in 0 .. nh - 1 and the step itself wrote slot n + nh - 1 at most."""
    hi_b, hi_p = {}, {}
    order, todo = [], [root]
    while todo:
        i = todo.pop()
        order.append(i)
        todo += [int(c) for c in wide["child"][i] if 0 <= c < EMPTY]
    for i in reversed(order):
        kids = [int(c) for c in wide["child"][i] if c != EMPTY]
        inner = [c for c in kids if c >= 0]
        best_b = best_p = -1
        for nh in range(0, len(kids) + 1):
            best_b = max(best_b, nh - 1)                    # relative to n; nh = 0: the old top, n - 1
            if nh:
                best_p = max(best_p, nh - 1)
                for c in inner:
                    best_b = max(best_b, nh - 1 + hi_b[c])  # entered with n + nh - 1 entries at most
                    best_p = max(best_p, nh - 1 + hi_p[c])
        hi_b[i], hi_p[i] = best_b, best_p
    return hi_b[root], hi_p[root]


def audit(nodes, nodes32, roots, wide, levels):
    if len(wide) != len(nodes):
        raise AuditError("shape", "%d wide records for %d nodes" % (len(wide), len(nodes)))
    lo32, hi32 = wt.round_out(nodes["bmin"], nodes["bmax"])
    if not (np.array_equal(_bits(lo32), _bits(nodes32["lo"])) and np.array_equal(_bits(hi32), _bits(nodes32["hi"]))):
        raise AuditError("nodes32", "FlatNode32 planes are not the f64 planes rounded outward")
    reached = np.zeros(len(nodes), dtype=bool)
    top_b = top_p = 0  # highest slot written, absolute
    for root in roots:
        if root < 0:
            continue  # a BVH of one leaf: the walkers start at the leaf code; no record, no stack
        span = _leaf_spans(nodes, root)
        todo = [root]
        while todo:
            i = todo.pop()
            if reached[i]:
                raise AuditError("cut", "wide node %d is reached twice" % i)
            reached[i] = True
            w = wide[i]
            want = expected_slots(nodes, i)
            occupied = [k for k in range(4) if w["child"][k] != EMPTY]
            if occupied != list(range(len(occupied))):
                raise AuditError("empty", "node %d: an empty slot before an occupied one" % i)
            # the cut, from the records alone: each child sits one to three levels below i and the leaves tile i's
            below = {}
            level = [(i, 0), (i, 1)]
            for depth in (1, 2, 3):
                nxt = []
                for pos in level:
                    below.setdefault(int(nodes["child"][pos]), []).append(pos)
                    if nodes["child"][pos] >= 0:
                        nxt += [(int(nodes["child"][pos]), 0), (int(nodes["child"][pos]), 1)]
                level = nxt
            got = []
            for k in occupied:
                code = int(w["child"][k])
                if code not in below or len(below[code]) != 1:
                    raise AuditError("cut", "node %d slot %d: code %d is not a child one to three levels below" % (i, k, code))
                got.append(below[code][0])
            spans = sorted(span[pos] for pos in got)
            whole = (min(span[(i, 0)][0], span[(i, 1)][0]), max(span[(i, 0)][1], span[(i, 1)][1]))
            if spans[0][0] != whole[0] or spans[-1][1] != whole[1] or any(a[1] != b[0] for a, b in zip(spans, spans[1:])):
                raise AuditError("cut", "node %d: the children's leaves do not partition the node's" % i)
            if got != want:
                raise AuditError("order", "node %d: children %s, the definition gives %s" % (i, got, want))
            for k, (p, c) in enumerate(got):
                for a in range(3):
                    if _bits(w["lo"][a, k]) != _bits(nodes32["lo"][p, c, a]) or _bits(w["hi"][a, k]) != _bits(nodes32["hi"][p, c, a]):
                        raise AuditError("planes", "node %d slot %d axis %d: not the FlatNode32 planes of node %d child %d" % (i, k, a, p, c))
                    if w["lo"][a, k] > nodes["bmin"][p, c, a] or w["hi"][a, k] < nodes["bmax"][p, c, a]:
                        raise AuditError("planes", "node %d slot %d axis %d: does not enclose the f64 box" % (i, k, a))
            for k in range(len(occupied), 4):
                if not (np.all(w["lo"][:, k] == np.inf) and np.all(w["hi"][:, k] == -np.inf)):
                    raise AuditError("empty", "node %d slot %d: an empty slot's box is not (+inf, -inf)" % (i, k))
            if np.any(w["pad"] != 0):
                raise AuditError("empty", "node %d: pad words not 0" % i)
            todo += [int(c) for c in w["child"] if 0 <= c < EMPTY]
        hb, hp = stack_peaks(wide, root)
        top_b, top_p = max(top_b, 1 + hb), max(top_p, hp)
    raw = np.ascontiguousarray(wide).view(np.uint8).reshape(len(wide), 128)
    stray = np.nonzero(~reached & raw.any(axis=1))[0]
    if len(stray):
        raise AuditError("unreached", "node %d is reached by no wide walk and its record is not zero" % stray[0])
    if not any(r >= 0 for r in roots):
        if levels != 1:
            raise AuditError("levels", "no tree to walk: %d levels, slot 0 alone is needed" % levels)
        return {"levels": levels, "wide_nodes": 0}
    if top_b != levels - 1:
        raise AuditError("levels", "LdsStackB's highest slot is %d, levels - 1 is %d" % (top_b, levels - 1))
    if top_p != levels - 2:
        raise AuditError("levels", "LdsStack's highest slot is %d, levels - 2 is %d" % (top_p, levels - 2))
    return {"levels": levels, "wide_nodes": int(reached.sum())}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_tree")
    return wt.build_host_check(d), d


@pytest.mark.parametrize("case_id", list(wt.CASES))
def test_the_collapse_is_the_tree_its_definition_describes(rtsr, host_check, case_id):
    exe, d = host_check
    c = wt.case(rtsr, case_id)
    wide, levels = wt.run_host_check(exe, d, case_id, c["nodes"], c["roots"])
    got = audit(c["nodes"], c["nodes32"], c["roots"], wide, levels)
    print(case_id, "nodes", len(c["nodes"]), "roots", c["roots"], got)
    assert len(c["roots"]) >= 1
    if case_id == "two_triangle_bvh":  # the builder forces a node: one node of two one-triangle leaves
        assert len(c["roots"]) == 2 and min(c["roots"]) >= 0 and len(c["nodes"]) == 300
        assert [int(x) for x in wide["child"][c["roots"][0]]] == [wt.make_leaf(0, 1), wt.make_leaf(1, 1), EMPTY, EMPTY]
    if case_id == "two_bvhs":
        assert len(c["roots"]) == 2 and min(c["roots"]) >= 0
    if case_id.startswith("inner_"):
        n = int(case_id[-1])
        assert len(c["nodes"]) == n and int((wide["child"][c["roots"][0]] != EMPTY).sum()) == min(4, n + 1)
    if case_id == "comb":
        assert levels > 64  # three more entries per wide level: deeper than any LDS stack, the audit's recursion must not be Python's
    if case_id == "ties_and_odd_areas":
        assert [int(x) for x in wide["child"][0]] == [wt.make_leaf(0, 1), 2, 4, wt.make_leaf(1, 1)]
        assert [int(x) for x in wide["child"][2]] == [wt.make_leaf(4, 1), 6, wt.make_leaf(5, 1), EMPTY]  # the NaN area stays shut
        assert [int(x) for x in wide["child"][6]] == [wt.make_leaf(6, 1), wt.make_leaf(8, 1), wt.make_leaf(7, 1), 9]  # area 0 opened
        assert got["wide_nodes"] == 5


def test_the_self_run_of_the_host_check_is_clean(host_check):
    """No arguments: a comb, a root that is a leaf code beside it and alone (plan_wide's loop read nodes[root] with a negative
    root before build_wide_nodes learned to return at once), no tree at all."""
    import os
    import subprocess
    exe, _ = host_check
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **wt.SAN_ENV), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "wide tree host check clean" in out.stdout and "root leaf alone: 1 levels" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_make_sanitize_builds_the_host_check_and_its_own_run_is_clean():
    import os
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(wt.ROOT, "oracle"), "sanitize"], check=True)
    env = dict(os.environ, **wt.SAN_ENV)
    out = subprocess.run([os.path.join(wt.ROOT, "oracle", "_build", "wide_tree_host_check")], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "wide tree host check clean" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for name in ("wide_step_host_check", "wide_step_host_check_f32"):
        assert os.path.exists(os.path.join(wt.ROOT, "oracle", "_build", name))


def _swap_slots(w, i, a, b):
    for f in ("lo", "hi"):
        w[f][i][:, [a, b]] = w[f][i][:, [b, a]]
    w["child"][i][[a, b]] = w["child"][i][[b, a]]


@pytest.mark.parametrize("case_id", ["dragon_2000", "ties_and_odd_areas"])
def test_the_audit_names_each_corruption(rtsr, host_check, case_id):
    exe, d = host_check
    c = wt.case(rtsr, case_id)
    wide, levels = wt.run_host_check(exe, d, case_id + "_selftest", c["nodes"], c["roots"])
    audit(c["nodes"], c["nodes32"], c["roots"], wide, levels)
    root = c["roots"][0]
    full = [i for i in range(len(wide)) if np.all(wide["child"][i] != EMPTY) and wide["child"][i][0] != 0]
    part = [i for i in range(len(wide)) if wide["child"][i][3] == EMPTY and wide["child"][i][0] != wide["child"][i][3]]

    def expect(kind, change):
        w = wide.copy()
        lv = change(w)
        with pytest.raises(AuditError) as e:
            audit(c["nodes"], c["nodes32"], c["roots"], w, levels if lv is None else lv)
        assert e.value.kind == kind, str(e.value)

    def inward(w):  # one plane moved inward by an ulp
        w["lo"][root][1, 0] = np.nextafter(w["lo"][root][1, 0], np.float32(np.inf))
    expect("planes", inward)

    def inward_hi(w):
        i = full[-1]
        w["hi"][i][2, 3] = np.nextafter(w["hi"][i][2, 3], np.float32(-np.inf))
    expect("planes", inward_hi)
    expect("order", lambda w: _swap_slots(w, full[0], 1, 2))

    def clear_code(w):
        w["child"][part[0]][3] = 0
    if part:
        expect("cut", clear_code)

        def box_of_empty(w):
            w["lo"][part[0]][0, 3] = np.float32(0.0)
        expect("empty", box_of_empty)
    else:
        assert case_id != "ties_and_odd_areas"
    expect("levels", lambda w: levels - 1)
    expect("levels", lambda w: levels + 1)

    def stray(w):
        free = [i for i in range(len(w)) if not np.ascontiguousarray(w[i:i + 1]).view(np.uint8).any()]
        if free:
            w["pad"][free[0]][2] = 1
            return None
        w["pad"][root][2] = 1
    expect("unreached" if np.any(~np.ascontiguousarray(wide).view(np.uint8).reshape(len(wide), 128).any(axis=1)) else "empty", stray)

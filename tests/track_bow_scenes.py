"""track_bow_scenes.py -- hand-made scenes for the batched TrackReferenceKeyFrame matcher (test infrastructure only), shared by
tests/test_track_bow_cpu.py (restatement against the C oracle, scene coverage) and tests/test_gpu_track_bow.py (ivf_tracker_search_by_bow
against both).  Everything is drawn from fixed seeds.

The trees (branching 3..5, depth 3 and 4, one leaf above the last level) are built so that a descriptor's path is chosen by hand:
bytes 2l, 2l + 1 of a descriptor are the "address" of level l + 1, one of five 16-bit codes that differ in at least 8 bits; a node's
descriptor holds its own code and zeros elsewhere, so siblings differ in their level's two bytes only and the descent follows the address
exactly.  Bytes 8..31 (192 bits) are payload: descriptors of one address differ by exactly the payload bits that were flipped."""
import numpy as np

import track_bow_ref as R

F = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # ivf_keypoint
NF = 256                                                       # nfeatures of the tracker the scenes are packed for
CODES = (0x0000, 0x00FF, 0xFF00, 0x0F0F, 0xF0F0)
W, H = 640.0, 240.0
CAM = dict(fx=F(370.0), fy=F(370.0), cx=F(320.0), cy=F(120.0), bf=F(198.75))
BOUNDS = (0.0, 0.0, W, H)


def make_tree(depth, seed):
    """-> dict(child_start, child, desc, word, weight, depth, children): the flat arrays ivf_vocabulary_create / orc_bow_transform take.
    Level-1 child 2 is a leaf (features sent there have no node at level >= 2: node id 0); the last leaf is a stopped word."""
    rng = np.random.default_rng(seed)
    children = [[]]; level = [0]; code = [0]; frontier = [0]
    for lv in range(1, depth + 1):
        nxt = []
        for node in frontier:
            if lv == 2 and code[node] == CODES[2]:
                continue
            k = 5 if lv == 1 else int(rng.integers(3, 6))
            if lv == 2 and code[node] != CODES[4]:
                k = 5
            for c in range(k):
                children.append([]); level.append(lv); code.append(CODES[c]); children[node].append(len(children) - 1); nxt.append(len(children) - 1)
        frontier = nxt
    n = len(children)
    start = np.zeros(n + 1, np.int32); flat = []
    for i in range(n):
        flat.extend(children[i]); start[i + 1] = len(flat)
    desc = np.zeros((n, 32), np.uint8)
    for i in range(1, n):
        desc[i, 2 * (level[i] - 1)] = code[i] & 0xFF; desc[i, 2 * (level[i] - 1) + 1] = code[i] >> 8
    word = np.full(n, -1, np.int32); weight = np.zeros(n, np.float64); w = 0
    for i in range(n):
        if not children[i]:
            word[i] = w; w += 1; weight[i] = float(rng.uniform(0.1, 9.0))
    stopped = max(i for i in range(n) if not children[i])
    weight[stopped] = 0.0
    return dict(child_start=start, child=np.array(flat, np.int32), desc=desc, word=word, weight=weight, depth=depth, children=children,
                n_words=w, stopped=stopped)


TREES = {3: make_tree(3, 11), 4: make_tree(4, 12)}


def path_of(tree, prefix):
    """prefix (c1, c2, ...) extended by first children down to a leaf -> (full path, node ids along it)"""
    node = 0; path = []; ids = []
    for c in prefix:
        node = tree["children"][node][c]; path.append(c); ids.append(node)
    while tree["children"][node]:
        node = tree["children"][node][0]; path.append(0); ids.append(node)
    return path, ids


def path_to(tree, target):
    """the path that ends at node `target`"""
    def walk(node, path):
        if node == target:
            return path
        for c, ch in enumerate(tree["children"][node]):
            r = walk(ch, path + [c])
            if r is not None:
                return r
        return None
    return walk(0, [])


class Builder:
    """collects the keyframe's and the frame's features of one scene; payloads are 192-bit patterns, flips name payload bit positions"""

    def __init__(self, tree, seed):
        self.tree = tree; self.rng = np.random.default_rng(seed)
        self.kf = []; self.f = []
        # level-2 prefixes in ascending node-id order (level-1 child 2 is a leaf: its features carry node id 0 at any level >= 2)
        self.nodes = [(c1, c2) for c1 in range(5) if c1 != 2 for c2 in range(len(tree["children"][tree["children"][0][c1]]))]
        self.next = 0

    def node(self):
        self.next += 1
        return self.nodes[self.next - 1]

    def payload(self):
        return self.rng.integers(0, 256, 24, dtype=np.uint8)

    def flipped(self, payload, bits):
        p = payload.copy()
        for b in bits:
            p[b // 8] ^= np.uint8(1 << (b % 8))
        return p

    def pick(self, n, avoid=()):
        free = [b for b in range(192) if b not in set(avoid)]
        return [int(b) for b in self.rng.permutation(free)[:n]]

    def desc(self, prefix, payload):
        path, _ = path_of(self.tree, prefix) if not isinstance(prefix, list) else (prefix, None)
        d = np.zeros(32, np.uint8)
        for l, c in enumerate(path):
            d[2 * l] = CODES[c] & 0xFF; d[2 * l + 1] = CODES[c] >> 8
        d[8:] = payload
        return d

    def add_kf(self, prefix, payload, has=1, angle=0.0):
        self.kf.append((self.desc(prefix, payload), has, angle)); return len(self.kf) - 1

    def add_f(self, prefix, payload, angle=0.0):
        self.f.append((self.desc(prefix, payload), angle)); return len(self.f) - 1

    def good(self, prefix, n, flips=3, kf_angle=0.0, f_angle=0.0):
        """n keyframe features and their twins in the frame (payload with `flips` bits flipped), the frame's in reverse order"""
        ps = [self.payload() for _ in range(n)]
        for p in ps:
            self.add_kf(prefix, p, angle=kf_angle)
        for p in reversed(ps):
            self.add_f(prefix, self.flipped(p, self.pick(flips)), angle=f_angle)

    def side(self, items, with_has):
        n = len(items)
        assert n <= NF
        kp = np.zeros(n, KP_DTYPE)
        kp["x"] = self.rng.uniform(20, W - 20, n).astype(F); kp["y"] = self.rng.uniform(20, H - 20, n).astype(F); kp["size"] = 31
        kp["angle"] = np.array([it[-1] for it in items], F)
        out = dict(kps=kp, desc=np.array([it[0] for it in items], np.uint8).reshape(n, 32))
        if with_has:
            out["has"] = np.array([it[1] for it in items], np.uint8)
        return out

    def scene(self, name, levelsup):
        return dict(name=name, tree=self.tree, levelsup=levelsup, kf=self.side(self.kf, True), f=self.side(self.f, False))


def main_scene(tree, levelsup, seed=1):
    """every gate of the match at nodes of their own; nodes on one side only at the front (node 0), in the middle and at the end"""
    b = Builder(tree, seed)
    leaf = [2]                                                              # the leaf above the last level: node id 0, front of both lists
    for _ in range(3):
        b.add_kf(leaf, b.payload())                                         # keyframe only, at the front
    b.good(b.node(), 12)
    nd = b.node()                                                           # frame only, right behind
    for _ in range(2):
        b.add_f(nd, b.payload())
    b.good(b.node(), 12, kf_angle=5.0, f_angle=355.0)                       # rot = -350 before the + 360, bin 0
    nd = b.node(); p = b.payload()                                          # distance exactly 50: accepted
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(50)))
    nd = b.node(); p = b.payload()                                          # distance exactly 51: over TH_LOW
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(51)))
    nd = b.node(); p = b.payload()                                          # ratio gate, passing side: 20 < 0.7 * 29
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(29))); b.add_f(nd, b.flipped(p, b.pick(20)))
    nd = b.node(); p = b.payload()                                          # ratio gate, failing side: 22 >= 0.7 * 30
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(22))); b.add_f(nd, b.flipped(p, b.pick(30)))
    nd = b.node(); p = b.payload()                                          # keyframe-only node in the middle
    b.add_kf(nd, p)
    nd = b.node()                                                           # frame-only node in the middle
    b.add_f(nd, b.payload())
    nd = b.node(); p = b.payload()                                          # two frame features at the same best distance: the first wins, the ratio fails
    b.add_kf(nd, p); b.add_f(nd, b.flipped(p, b.pick(10))); b.add_f(nd, b.flipped(p, b.pick(10)))
    nd = b.node(); p = b.payload()                                          # two keyframe features want the same frame feature: the second takes its next best
    x = b.pick(2); y = b.pick(1, avoid=x); z = b.pick(30, avoid=x + y)
    b.add_kf(nd, p); b.add_kf(nd, b.flipped(p, x))
    b.add_f(nd, b.flipped(p, x + z)); b.add_f(nd, b.flipped(p, y))           # distances (32, 30) and (1, 3)
    nd = b.node(); p = b.payload()                                          # ... or fails: its next best is over TH_LOW
    x = b.pick(2); y = b.pick(1, avoid=x); z = b.pick(60, avoid=x + y)
    b.add_kf(nd, p); b.add_kf(nd, b.flipped(p, x))
    b.add_f(nd, b.flipped(p, y)); b.add_f(nd, b.flipped(p, x + z))
    nd = b.node(); p = b.payload()                                          # ... or finds every candidate taken
    b.add_kf(nd, p); b.add_kf(nd, b.flipped(p, b.pick(2))); b.add_f(nd, b.flipped(p, b.pick(1)))
    nd = b.node(); p = b.payload(); q = b.payload()                         # a keyframe feature without a map point, its twin stays free
    b.add_kf(nd, p, has=0); b.add_kf(nd, q); b.add_f(nd, p); b.add_f(nd, b.flipped(q, b.pick(4)))
    nd = b.node(); p = b.payload()                                          # one match in a bin of its own (rot = 150): taken back
    b.add_kf(nd, p, angle=200.0); b.add_f(nd, b.flipped(p, b.pick(2)), angle=50.0)
    # a stopped word: the features sent to that leaf are in no node
    sp = path_to(tree, tree["stopped"]); p = b.payload()
    b.add_kf(sp, p); b.add_f(sp, p)
    nd = b.nodes[-2]                                                        # frame only, near the end
    b.add_f(nd, b.payload())
    b.add_kf(b.nodes[-1], b.payload())                                      # keyframe only, at the end
    return b.scene("main", levelsup)


def swapped_ends_scene(tree, levelsup, seed=2):
    """the other lower_bound branch at the ends: the frame's list starts and ends with nodes the keyframe does not have"""
    b = Builder(tree, seed)
    b.add_f([2], b.payload())
    b.add_kf(b.node(), b.payload())
    b.good(b.node(), 5)
    b.add_f(b.node(), b.payload())
    b.good(b.node(), 5, kf_angle=90.0, f_angle=90.0)
    b.add_kf(b.nodes[-3], b.payload())
    b.add_f(b.nodes[-2], b.payload())
    return b.scene("swapped_ends", levelsup)


def wide_nodes_scene(tree, levelsup, seed=3):
    """a node with more than 64 frame features (matches and a ratio test whose two distances sit in different strides of 64) and a node
    with more than 64 keyframe features (claims across the 64-feature chunks)"""
    b = Builder(tree, seed)
    nd = b.node()
    ps = [b.payload() for _ in range(4)]
    fill = [b.payload() for _ in range(70)]
    fill[2] = b.flipped(ps[0], b.pick(3)); fill[65] = b.flipped(ps[1], b.pick(4)); fill[69] = b.flipped(ps[2], b.pick(5))
    fill[5] = b.flipped(ps[3], b.pick(20)); fill[68] = b.flipped(ps[3], b.pick(25))      # 20 >= 0.7 * 25: fails across the strides
    for p in ps:
        b.add_kf(nd, p)
    for p in fill:
        b.add_f(nd, p)
    nd = b.node()
    ks = [b.payload() for _ in range(70)]
    for p in ks:
        b.add_kf(nd, p)
    for j in (69, 64, 63, 0, 30):
        b.add_f(nd, b.flipped(ks[j], b.pick(3)))
    b.add_f(nd, b.flipped(ks[64], b.pick(4)))                              # a second twin of 64: 3 >= 0.7 * 4 fails the ratio, nobody takes either
    return b.scene("wide_nodes", levelsup)


def one_node_scene(tree, seed=4):
    """levelsup >= L: every feature in node 0, one long serial chain with more than 64 features on both sides"""
    b = Builder(tree, seed)
    ks = []
    for j in range(80):
        nd = b.nodes[j % len(b.nodes)]; p = b.payload(); ks.append((nd, p))
        b.add_kf(nd, p, has=0 if j % 9 == 4 else 1, angle=float(7 * j % 360))
    order = b.rng.permutation(80)
    for j in order[:60]:
        nd, p = ks[j]
        b.add_f(nd, b.flipped(p, b.pick(int(b.rng.integers(0, 12)))), angle=float((7 * j + (3 if j % 5 else (200, 100, 40, 290)[(j // 5) % 4])) % 360))
    for j in range(30):
        b.add_f(b.nodes[j % 7], b.payload(), angle=11.0)
    return b.scene("one_node", tree["depth"])


def rotation_scene(tree, levelsup, bins, name, seed=5):
    """accepted matches spread over rotation bins: bins = [(rot in degrees, count)]; half of each bin's matches reach their rot through a
    negative difference"""
    b = Builder(tree, seed)
    k = 0
    for rot, count in bins:
        nd = b.nodes[k % len(b.nodes)]; k += 1
        for j in range(count):
            p = b.payload()
            fa = 40.0 + j if j % 2 else 300.0 - j                            # frame angle; keyframe angle = frame angle + rot (mod 360)
            ka = fa + rot
            if ka >= 360.0:
                ka -= 360.0                                                  # then rot is negative before the + 360
            b.add_kf(nd, p, angle=ka); b.add_f(nd, b.flipped(p, b.pick(2)), angle=fa)
    return b.scene(name, levelsup)


def empty_scene(tree, levelsup, which):
    b = Builder(tree, 6)
    b.good(b.node(), 3)
    if which == "f":
        b.f = []
    else:
        b.kf = []
    return b.scene("empty_" + which, levelsup)


def scenes(depth=3):
    """the scene set on the tree of that depth; levelsup puts the nodes at level 2"""
    tree = TREES[depth]; ls = depth - 2
    return [main_scene(tree, ls), swapped_ends_scene(tree, ls), wide_nodes_scene(tree, ls), one_node_scene(tree),
            rotation_scene(tree, ls, [(0.0, 25), (95.0, 2), (200.0, 1), (359.0, 1), (31.0, 1)], "rotation_one_bin"),
            rotation_scene(tree, ls, [(10.0, 12), (120.0, 8), (250.0, 5), (330.0, 3), (60.0, 1)], "rotation_three_bins"),
            empty_scene(tree, ls, "f"), empty_scene(tree, ls, "kf")]


def node_ids(O, sc, levelsup=None):
    """oracle_lib.bow_transform of both sides -> (keyframe feature vector, frame feature vector) as {node: [indices]}"""
    ls = sc["levelsup"] if levelsup is None else levelsup
    out = []
    for side in (sc["kf"], sc["f"]):
        if len(side["kps"]) == 0:
            out.append({}); continue
        _, nid, wt = O.bow_transform(sc["tree"], side["desc"], ls)
        out.append(R.feature_vector(nid, wt))
    return out


def oracle(O, sc, levelsup=None, nn_ratio=0.7, check_orientation=True, has=None):
    """orc_search_by_bow on the scene -> (f_match, nmatches)"""
    kfv, ffv = node_ids(O, sc, levelsup)
    return O.search_by_bow(sc["kf"]["kps"], sc["kf"]["desc"], sc["kf"]["has"] if has is None else has, kfv, sc["f"]["kps"], sc["f"]["desc"], ffv,
                           nn_ratio, check_orientation)


def records_of(sc, rng=None):
    """the two gather records of a scene: (keyframe, frame) as dict(kps, desc, uright, depth); a keyframe keypoint has a stereo depth
    exactly where it holds a map point (the default of ivf_tracker_search_by_bow without flags)"""
    out = []
    for side in (sc["kf"], sc["f"]):
        n = len(side["kps"])
        has = side.get("has", np.ones(n, np.uint8))
        depth = np.where(has != 0, 8.0, -1.0).astype(F)
        ur = np.where(has != 0, side["kps"]["x"] - CAM["bf"] / F(8.0), -1.0).astype(F)
        out.append(dict(kps=side["kps"], desc=side["desc"], uright=ur, depth=depth))
    return out

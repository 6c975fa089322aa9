"""Host helpers of the NMS / top-K selection tests (no GPU, no library): score maps whose result depends on values exactly
5 * radius pixels away, a tiled run of the oracle's simple_nms with a halo of the caller's choice, the score-map
families, and NumPy restatements of three rules of the product: the histogram bin of a score (key_bin,
sfd2_amd/csrc/sfd2_internal.h), the candidate capacity (cand_capacity, sfd2_amd/csrc/sfd2_ctx.h) and the tile height
launch_nms4_select (sfd2_amd/csrc/nms4_kernels.hip) picks for a map.

Why 5 * radius: simple_nms is one max-pool compare and two rounds of suppress / compare.  max_mask after round 2 at a
pixel t reads the suppressed scores within r of t; those read supp_mask, i.e. max_mask after round 1 within 2r; that
reads the suppressed scores of round 1 within 3r, their supp_mask within 4r, and the first max_mask reads scores within
5r.  A chain of six strictly decreasing values at pitch r realises the bound: p0 is a maximum, suppresses p1, which frees
p2, which suppresses p3, which frees p4, which suppresses p5.  Without p0 the survivors are p1, p3, p5 instead of p0, p2,
p4: the sixth point's fate is decided by the first one, 5r away."""
import numpy as np

from oracle import oracle as orc

def chain(m, y, x, dy, dx, pitch, n=6, top=0.9):
    """Writes n strictly decreasing values, top * (1 - 0.05 i), at (y + i pitch dy, x + i pitch dx) into m.  Returns the
    list of the points.  The caller keeps every point inside m."""
    pts = []
    for i in range(n):
        yy, xx = y + i * pitch * dy, x + i * pitch * dx
        assert 0 <= yy < m.shape[0] and 0 <= xx < m.shape[1], (yy, xx, m.shape)
        m[yy, xx] = np.float32(top * (1.0 - 0.05 * i))
        pts.append((yy, xx))
    return pts


def _seam_candidates(h, w, tile_h, tile_w, reach):
    """Every chain that ends on the first row / column of a tile behind an interior seam, as (group, y5, x5, dy, dx): the
    sixth point (y5, x5) and the direction the chain runs in; the first point lies `reach` = 5 * pitch before it.  A group
    is one seam and one side of it, or one seam crossing; candidates of a group differ in the position along the seam."""
    out = []
    xs = list(range(tile_w, w, tile_w))
    ys = list(range(tile_h, h, tile_h))
    for X in xs:
        for y in range(0, h, 7):
            out.append((("x", X, "from_left"), y, X, 0, 1))           # into the tile that starts at column X
            out.append((("x", X, "from_right"), y, X - 1, 0, -1))     # into the tile that ends at column X - 1
    for Y in ys:
        for x in range(0, w, 7):
            out.append((("y", Y, "from_top"), Y, x, 1, 0))
            out.append((("y", Y, "from_bottom"), Y - 1, x, -1, 0))
    for Y in ys:
        for X in xs:                                                     # the four tiles that meet at (Y, X)
            for (y5, x5, dy, dx) in ((Y, X, 1, 1), (Y, X - 1, 1, -1), (Y - 1, X, -1, 1), (Y - 1, X - 1, -1, -1)):
                out.append((("c", Y, X), y5, x5, dy, dx))
    ok = []
    for g, y5, x5, dy, dx in out:
        y0, x0 = y5 - reach * dy, x5 - reach * dx
        if 0 <= y0 < h and 0 <= x0 < w:
            ok.append((g, y5, x5, dy, dx))
    return ok


def seam_chains(h, w, tile_h, tile_w, radius, pitch=None, per_group=3, seed=0, corners_first=False):
    """Chains of six values at pitch `radius` across the interior tile seams of an h x w map cut into tile_h x tile_w tiles:
    for every seam chains that enter a tile from the left, right, top and bottom, and diagonal chains into the tile
    corners.  The first point sits 5 * radius outside the tile, the sixth on the tile's first row or column.  Chains keep
    a Chebyshev distance of more than 5 * radius + 4 from each other, so none changes another's result.

    Placement is greedy and deterministic: in each of per_group rounds every group (a seam and a side, or a crossing)
    gets the first of its candidates that fits, the search starting further along the seam in every round.  Seams come
    before crossings, so every seam side on which a chain fits gets one; the spacing rule then leaves room for a diagonal
    chain at some crossings only, on a small map at none.  corners_first places the crossings before the seams: as many
    diagonal chains as fit (with 24-row tiles at most every other crossing), seam sides where room is left.

    Returns (zero, noisy, anchors): the chains on a zero map, the same chains on a background uniform below 0.05, and
    one dict per chain with 'first' and 'sixth' (y, x), 'dir' (dy, dx) and 'group'."""
    pitch = radius if pitch is None else pitch
    reach = 5 * pitch
    gap = 5 * radius + 5
    cands = _seam_candidates(h, w, tile_h, tile_w, reach)
    groups = {}
    for c in sorted(cands, key=lambda c: c[0][0] != "c") if corners_first else cands:   # stable: order within a kind stays
        groups.setdefault(c[0], []).append(c)
    boxes = np.empty((len(groups) * per_group, 4), dtype=np.int64)   # (y_lo, y_hi, x_lo, x_hi) of the chains placed, inclusive
    nbox = 0

    def fits(b):
        q = boxes[:nbox]
        dy = np.maximum(np.maximum(q[:, 0] - b[1], b[0] - q[:, 1]), 0)
        dx = np.maximum(np.maximum(q[:, 2] - b[3], b[2] - q[:, 3]), 0)
        return not (np.maximum(dy, dx) < gap).any()

    zero = np.zeros((h, w), dtype=np.float32)
    anchors = []
    tops = (0.9, 0.8, 0.9, 0.7, 0.6, 0.8)   # equal tops on purpose: equal scores in different chains
    for rnd in range(per_group):
        for gi, (g, lst) in enumerate(groups.items()):
            start = (rnd * len(lst)) // per_group + (3 * gi) % max(1, len(lst) // per_group)
            for j in range(len(lst)):
                _, y5, x5, dy, dx = lst[(start + j) % len(lst)]
                y0, x0 = y5 - reach * dy, x5 - reach * dx
                b = (min(y0, y5), max(y0, y5), min(x0, x5), max(x0, x5))
                if not fits(b):
                    continue
                boxes[nbox] = b
                nbox += 1
                chain(zero, y0, x0, dy, dx, pitch, 6, tops[len(anchors) % len(tops)])
                anchors.append({"first": (y0, x0), "sixth": (y5, x5), "dir": (dy, dx), "group": g})
                break
    rs = np.random.RandomState(seed + 1000 * h + w)
    noisy = (0.05 * rs.random_sample((h, w))).astype(np.float32)
    noisy[zero > 0] = zero[zero > 0]
    return zero, noisy, anchors


def tiled_nms(m, tile_h, tile_w, halo, radius):
    """The oracle's simple_nms run per tile on the tile plus `halo` pixels on every side (clipped to the map), the tile
    interiors pasted together.  Equal to the untiled result when halo >= 5 * radius."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    h, w = m.shape
    out = np.empty_like(m)
    for y0 in range(0, h, tile_h):
        for x0 in range(0, w, tile_w):
            y1, x1 = min(y0 + tile_h, h), min(x0 + tile_w, w)
            cy0, cx0 = max(y0 - halo, 0), max(x0 - halo, 0)
            cy1, cx1 = min(y1 + halo, h), min(x1 + halo, w)
            r = orc.simple_nms(m[cy0:cy1, cx0:cx1], radius)
            out[y0:y1, x0:x1] = r[y0 - cy0:y1 - cy0, x0 - cx0:x1 - cx0]
    return out


FAMILIES = ("rand", "smooth", "plateau", "sparse", "const", "rampnoise", "quant", "wide", "sparse_plateau")


def family(kind, h, w, seed=0):
    """One score map of a named family, float32, read-only."""
    rs = np.random.RandomState(seed + 7 * h + w)
    u = rs.random_sample((h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (xx + yy) / float(h + w)
    if kind == "rand":
        m = u
    elif kind == "smooth":            # heat-map like: peaky, mostly tiny values
        m = u ** 12
    elif kind == "plateau":           # four levels: every 0.75 pixel is a maximum of its window
        m = np.floor(u * 4) / 4
    elif kind == "sparse":
        m = np.where(u > 0.97, rs.random_sample((h, w)), 0)
    elif kind == "const":
        m = np.full((h, w), 0.25)
    elif kind == "rampnoise":
        m = ramp + 0.02 * u
    elif kind == "quant":             # 64 levels of noise times a ramp: many near and exact ties along the anti-diagonals
        m = np.floor(u * 64) / 64 * ramp
    elif kind == "wide":              # scores over 28 octaves, below 2^-12 and above 16 (the clamped histogram bins); on a
        m = np.where(u > 0.9, 2.0 ** rs.uniform(-20, 8, (h, w)), 0)   # sparse support, or only the top octave survives the NMS
    elif kind == "sparse_plateau":    # three levels on 3 % of the pixels: equal scores, few enough for any capacity
        m = np.where(u > 0.97, np.floor(rs.random_sample((h, w)) * 3 + 1) / 4, 0)
    else:
        raise ValueError(kind)
    m = np.ascontiguousarray(m, dtype=np.float32)
    m.setflags(write=False)
    return m


HIST_BINS = 4096


def key_bin(score):
    """Histogram bin of a score (key_bin in sfd2_amd/csrc/sfd2_internal.h): the float32 bits below the sign, >> 15 (8
    exponent bits and the top 8 of the mantissa), rebased so that bin 0 starts at 2^-12, clamped to [0, 4095]."""
    bits = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    b = ((bits >> 15) & 0xFFFF).astype(np.int64) - ((127 - 12) << 8)
    return np.clip(b, 0, HIST_BINS - 1)


def capacity(n_pixels):
    """Candidates the selection keeps for a map of n_pixels (cand_capacity in sfd2_amd/csrc/sfd2_ctx.h)."""
    return min(max(65536, n_pixels // 8), n_pixels)


def nms4_tile(H, W):
    """'big' (96-row tile, nms4_select_kernel<136>) or 'small' (24 rows, <64>): the choice of launch_nms4_select in
    sfd2_amd/csrc/nms4_kernels.hip, restated.  It is used ONLY to assert that the shape lists of
    tests/test_gpu_selection_edges.py reach the tile they are named after -- whoever changes the launcher's rule changes
    this function with it and then revisits those lists (BIG_TILE_SHAPES, SMALL_TILE_SHAPES, TALL_SMALL_TILE_SHAPES)."""
    gx = (W + 87) // 88
    nb_s, nb_b = gx * ((H + 23) // 24), gx * ((H + 95) // 96)
    work_s = ((nb_s + 511) // 512) * 2 * 64      # region rows on the busiest CU: two 64-row blocks per CU ...
    work_b = ((nb_b + 255) // 256) * 136         # ... or one 136-row block
    return "big" if work_b < work_s else "small"

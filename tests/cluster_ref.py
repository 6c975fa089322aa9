"""Helpers shared by tests/golden/gen_cluster_goldens.py and the clustering tests (never imported by the product): a plain
restatement of the covisibility clustering as include/sfd2_hip.h specifies it, and seeded map generators."""
import numpy as np

from covis_ref import Img, Pt


def edges_of(frame_ids, images, points3D):
    """edge[a] = the set of ids of the list that a points at: b is in it when b occurs in the track of a point that a observes."""
    in_list = set(frame_ids)
    edge = {}
    for a in in_list:
        out = set()
        for p in np.asarray(images[a].point3D_ids).reshape(-1):
            if p != -1:
                out.update(int(b) for b in points3D[int(p)].image_ids if int(b) in in_list)
        edge[a] = out
    return edge


def clusters(frame_ids, images, points3D):
    """The specification: walk the list; a frame not yet visited opens a cluster holding every not-yet-visited frame of the list
    reachable from it over directed edges; then a stable sort by size, largest first; members by list position."""
    frame_ids = [int(f) for f in frame_ids]
    position = {}
    for p, f in enumerate(frame_ids):
        position.setdefault(f, p)
    edge = edges_of(frame_ids, images, points3D)
    visited, made = set(), []
    for seed in frame_ids:
        if seed in visited:
            continue
        members, frontier = {seed}, [seed]
        while frontier:
            a = frontier.pop()
            for b in edge[a]:
                if b not in visited and b not in members:
                    members.add(b)
                    frontier.append(b)
        visited |= members
        made.append(sorted(members, key=position.get))
    order = sorted(range(len(made)), key=lambda c: (-len(made[c]), c))
    return [made[c] for c in order]


# ---------------------------------------------------------------------------------------------------------------- maps
def build_map(n_images, tracks, first_id=1, first_point=10):
    """tracks: a list of (observers, track): the point occupies one key point in every image of `observers` and its image_ids are
    `track` (which may repeat images and may name images that do not observe it).  Image ids are first_id .. first_id + n_images - 1
    (indices in the arguments are 0-based); every image gets key points without a point (-1) too."""
    per_image = [[] for _ in range(n_images)]
    points3D = {}
    for p, (observers, track) in enumerate(tracks):
        pid = first_point + 3 * p
        for i in observers:
            per_image[i].append(pid)
        points3D[pid] = Pt(np.zeros(3), [first_id + int(i) for i in track])
    images = {}
    for i in range(n_images):
        ids = []
        for pid in per_image[i]:
            ids += [pid, -1]
        images[first_id + i] = Img(f"db/{i:05d}.jpg", [1.0, 0, 0, 0], [0.0, 0, 0], np.array(ids + [-1], dtype=np.int64))
    return images, points3D


def link(a, b):
    """One point seen by a and b: edges both ways."""
    return ([a, b], [a, b])


def chain_map(n, extra_images=0):
    """Images 0 .. n - 1 in a chain, each link a single point."""
    return build_map(n + extra_images, [link(i, i + 1) for i in range(n - 1)])


def planted_map(sizes, seed=0, noise_images=20, noise_points=60, repeats=True):
    """Components of the given sizes (a random spanning tree plus a few extra links each), then noise: images outside every component
    that share points among themselves only, tracks that list an image twice, and the last image observing nothing.  Returns (images,
    points3D, components as lists of 0-based indices)."""
    rs = np.random.RandomState(seed)
    tracks, comps, base = [], [], 0
    for s in sizes:
        comp = list(range(base, base + s))
        for j in range(1, s):
            tracks.append(link(comp[j], comp[rs.randint(0, j)]))
        for _ in range(s // 2):
            a, b = rs.choice(comp, 2) if s > 1 else (comp[0], comp[0])
            obs = sorted({int(a), int(b)})
            tracks.append((obs, obs + ([obs[0]] if repeats else [])))      # a repeated image in the track
        if s == 1:
            tracks.append(([comp[0]], [comp[0]]))                           # a track of length 1
        comps.append(comp)
        base += s
    noise = list(range(base, base + noise_images))
    for _ in range(noise_points):
        obs = sorted(set(int(v) for v in rs.choice(noise, 3)))
        tracks.append((obs, obs))
    images, points3D = build_map(base + noise_images + 1, tracks)
    return images, points3D, comps


def interleave(comps, seed=0):
    """A list holding every member of every component, shuffled, as 0-based indices."""
    rs = np.random.RandomState(seed)
    flat = [i for c in comps for i in c]
    return [flat[i] for i in rs.permutation(len(flat))]


def one_way_map():
    """Image 0 observes a point whose track lists 0 and 1; image 1 does not observe it (edge 0 -> 1 only).  Image 2 observes a point
    whose track lists 2 and 3 likewise, and 3 observes one that lists 3 and 0.  Image 4 is isolated, image 5 observes nothing."""
    return build_map(6, [([0], [0, 1]), ([2], [2, 3]), ([3], [3, 0]), ([4], [4])])


GOLDEN_CASES = {  # name: (map builder, list of 0-based index lists)
    "planted": lambda: (planted_map([5, 3, 3, 2, 2, 1], seed=1)[:2], [interleave(planted_map([5, 3, 3, 2, 2, 1], seed=1)[2], s) for s in range(4)]
                        + [[0, 5, 5, 1, 0, 8, 6, 30, 31, 6]]),
    "chain": lambda: (chain_map(40, 3), [list(np.random.RandomState(2).permutation(40)), list(range(0, 40, 2)), [7, 8, 9, 20, 41, 21, 42]]),
    "one_way": lambda: (one_way_map(), [[0, 1, 2, 3, 4, 5], [1, 0, 3, 2, 5, 4], [3, 0, 1], [1, 3, 0], [5], [2, 3, 0, 1]]),
}


def golden_inputs(name):
    """(images, points3D, lists of image ids) of a golden case."""
    (images, points3D), lists = GOLDEN_CASES[name]()
    return images, points3D, [[int(i) + 1 for i in li] for li in lists]

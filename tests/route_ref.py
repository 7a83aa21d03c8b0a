"""The goal fields of include/neupan_amd.h ("goal fields") restated: a heap Dijkstra over the same moves, costs and diagonal
rule on Python integers, the maps the route tests run on, and the doorway scene of the closed-loop test.  Nothing here
imports the package: the tests compare the package with this."""
import heapq

import numpy as np

BLOCKED, UNREACHED = 0xFFFFFFFF, 0xFFFFFFFE
MOVES = ((1, 0, 5), (-1, 0, 5), (0, 1, 5), (0, -1, 5), (1, 1, 7), (-1, 1, 7), (1, -1, 7), (-1, -1, 7))    # E W N S NE NW SE SW


def dijkstra(blocked, seeds):
    """blocked [ny, nx] (non-zero: not traversable; everything outside too); seeds: {(i, j): value}.  Returns the field as a
    uint32 array [ny, nx]: BLOCKED in blocked cells, UNREACHED where no move sequence leads, else min over the seeds of value +
    cost.  A diagonal move needs both axis cells beside it free."""
    occ = np.asarray(blocked) != 0
    ny, nx = occ.shape
    rows = occ.tolist()
    free = lambda i, j: 0 <= i < nx and 0 <= j < ny and not rows[j][i]
    best = {}
    heap = []
    for (i, j), v in seeds.items():
        assert free(i, j), (i, j)
        heap.append((int(v), i, j))
    heapq.heapify(heap)
    while heap:
        v, i, j = heapq.heappop(heap)
        if (i, j) in best:
            continue
        best[(i, j)] = v
        for di, dj, c in MOVES:
            a, b = i + di, j + dj
            if (a, b) in best or not free(a, b):
                continue
            if di and dj and not (free(i + di, j) and free(i, j + dj)):
                continue
            heapq.heappush(heap, (v + c, a, b))
    out = np.full((ny, nx), UNREACHED, dtype=np.uint32)
    out[occ] = BLOCKED
    for (i, j), v in best.items():
        out[j, i] = v
    return out


def dijkstra_moves(blocked, seeds):
    """dijkstra ordered by (cost, moves): returns (field, moves [ny, nx] int64) -- moves[j, i] is the least number of moves among
    the cheapest move sequences from a seed to (i, j), -1 where the cell is blocked or unreached.  (cost, moves) adds along a
    sequence and is ordered lexicographically, so the heap argument is Dijkstra's.)  The header's claim about k sweeps short
    of convergence is about exactly these cells: moves <= k."""
    occ = np.asarray(blocked) != 0
    ny, nx = occ.shape
    rows = occ.tolist()
    free = lambda i, j: 0 <= i < nx and 0 <= j < ny and not rows[j][i]
    best = {}
    heap = [(int(v), 0, i, j) for (i, j), v in seeds.items()]
    heapq.heapify(heap)
    while heap:
        v, m, i, j = heapq.heappop(heap)
        if (i, j) in best:
            continue
        best[(i, j)] = (v, m)
        for di, dj, c in MOVES:
            a, b = i + di, j + dj
            if (a, b) in best or not free(a, b):
                continue
            if di and dj and not (free(i + di, j) and free(i, j + dj)):
                continue
            heapq.heappush(heap, (v + c, m + 1, a, b))
    out = np.full((ny, nx), UNREACHED, dtype=np.uint32)
    out[occ] = BLOCKED
    moves = np.full((ny, nx), -1, dtype=np.int64)
    for (i, j), (v, m) in best.items():
        out[j, i], moves[j, i] = v, m
    return out, moves


# ---------------------------------------------------------------------------------------------------- the maps
def random_map(nx, ny, seed, share=0.2):
    """nx x ny, `share` of the cells blocked, seeded"""
    return (np.random.default_rng(seed).random((ny, nx)) < share).astype(np.uint8)


def pillars():
    """24 x 24 of single-cell pillars, 22 % of the cells, with the goal cell (12, 12) freed: starts all round the goal, chains
    that squeeze past corners, and many cells with several allowed moves"""
    occ = (np.random.default_rng(0).random((24, 24)) < 0.22).astype(np.uint8)
    occ[12, 12] = 0
    return occ


# (nx, ny, seed, goal cell) of the maps that end on, one past and one short of the 16-cell tile; the goals of the first three
# are corner cells of the map.  The seeds are the first at which the field reaches over 70 % of the cells and leaves some out
TILE_EDGE_MAPS = ((16, 16, 2, (15, 15)), (17, 16, 1, (16, 0)), (16, 17, 2, (0, 16)), (15, 33, 1, (7, 20)), (32, 16, 1, (16, 8)))


def tile_edge_map(nx, ny, seed, goal):
    occ = random_map(nx, ny, seed)
    occ[goal[1], goal[0]] = 0
    return occ


# the seeds of the large-seed runs over an open 9 x 7 map: every value above 2^31, and values on both sides of it
BIG_SEED = 2 ** 32 - 7 * 2 ** 26 - 1
BIG_SEEDS = ({(4, 3): BIG_SEED}, {(0, 0): 2 ** 31 - 3, (8, 6): 2 ** 31 - 23})


def inner_wall():
    """37 x 21 (neither a multiple of the 16-cell tile): a wall with a gap near the top, a stub from the bottom"""
    occ = np.zeros((21, 37), dtype=np.uint8)
    occ[0:17, 18] = 1
    occ[5, 3:12] = 1
    occ[12:21, 27] = 1
    return occ


def serpentine(n=48, lane=2):
    """n x n: walls one cell thick every lane + 1 rows, open for one cell at alternating ends -- the only path from the bottom
    row to the top runs the whole width of every lane, so it crosses every 16-cell tile several times"""
    occ = np.zeros((n, n), dtype=np.uint8)
    for k, j in enumerate(range(lane, n, lane + 1)):
        occ[j, :] = 1
        occ[j, n - 1 if k % 2 == 0 else 0] = 0
    return occ


def corner_pair():
    """9 x 7: the goal (0, 0) behind two blocked cells that touch at a corner, (1, 0) and (0, 1) -- the diagonal between them is
    the only way in and is forbidden, so every other free cell is UNREACHED"""
    occ = np.zeros((7, 9), dtype=np.uint8)
    occ[0, 1] = occ[1, 0] = 1
    return occ


def pocket():
    """20 x 18: a sealed room in the middle (walls one cell thick, free inside) and a goal outside it"""
    occ = np.zeros((18, 20), dtype=np.uint8)
    occ[5, 6:14] = occ[12, 6:14] = 1
    occ[5:13, 6] = occ[5:13, 13] = 1
    return occ


def tile_corner():
    """40 x 40 with a few pillars: the goal sits in the corner cell (15, 15) of the first 16-cell tile, next to three others;
    the pillars (16, 14) and (17, 15) touch at a corner, and the cheapest way from (16, 15) to (17, 14) is not between them"""
    occ = np.zeros((40, 40), dtype=np.uint8)
    occ[14, 16] = occ[15, 17] = occ[17, 14] = 1
    occ[20:30, 25] = 1
    occ[8, 2:9] = 1
    return occ


# name -> (occupancy [ny, nx], goal cell (i, j))
MAPS = {
    "1x1": (np.zeros((1, 1), dtype=np.uint8), (0, 0)),
    "1x23": (np.zeros((23, 1), dtype=np.uint8), (0, 4)),
    "23x1": (np.zeros((1, 23), dtype=np.uint8), (19, 0)),
    "inner_wall": (inner_wall(), (3, 2)),
    "serpentine": (serpentine(), (0, 0)),
    "corner_pair": (corner_pair(), (0, 0)),
    "pocket": (pocket(), (2, 3)),
    "tile_corner": (tile_corner(), (15, 15)),
}
_FIELDS = {}


def field(name, goal=None):
    """the Dijkstra field of a map of MAPS for its goal (or another goal cell), computed once"""
    occ, g = MAPS[name]
    g = tuple(goal) if goal is not None else g
    if (name, g) not in _FIELDS:
        _FIELDS[(name, g)] = dijkstra(occ, {g: 0})
        _FIELDS[(name, g)].setflags(write=False)
    return _FIELDS[(name, g)]


# ---------------------------------------------------------------------------------------------------- the doorway scene
DOOR_RES, DOOR_ORIGIN = 0.25, (0.0, 0.0)
DOOR_START, DOOR_GOAL = (1.5, 1.5, 0.0), (10.5, 1.5, 0.0)


def door_scene(doorway=4.0):
    """The 12 m x 8 m scene of the closed-loop test: 48 x 32 cells of 0.25 m, a wall two cells thick at x = 5.75 .. 6.25 m from the
    bottom edge up, open for `doorway` metres below the top edge; start and goal at y = 1.5 m on either side, so the straight
    line between them runs into the wall."""
    occ = np.zeros((32, 48), dtype=np.uint8)
    occ[:32 - int(round(doorway / DOOR_RES)), 23:25] = 1
    return occ

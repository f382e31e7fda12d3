"""Confined diffusion on filament geometries (the reference's unfinished mitochondria simulator,
Experiments/mitochondria_simulation/mitochnodria.py): a particle moves along a polyline, driven by 1-D displacements.

Edge, Geometry and draw_trajectory mirror the reference's public surface; pack_geometries is THE host function that turns
polylines into the arrays the kernel (csrc/confine.hip, ops.map_displacements) and its numpy restatement (_map_host) share;
map_displacements is the front end for several geometries at once; disp_fbm makes the displacements; cristae_geometry builds
the serpentine of cristae.  The arithmetic is stated once, in include/mivit_hip.h (mivit_map_displacements): kernel and
restatement are bitwise equal, and in clamp mode bitwise equal to the reference's loop."""
import math

import numpy as np
import torch

BOUNDARIES = ("clamp", "reflect")


class Edge:
    """A straight segment from start_point to end_point, (x, y) each.  length is np.linalg.norm of vector = end - start, angle
    its atan2 in radians; predecessor / ancestor are the neighbours a Geometry wires in; color is what Geometry.draw uses."""

    def __init__(self, start_point, end_point, predecessor=None, ancestor=None, color="blue"):
        self._start_point = np.array(start_point, dtype=float)
        self._end_point = np.array(end_point, dtype=float)
        if self._start_point.shape != (2,) or self._end_point.shape != (2,):
            raise ValueError(f"an edge needs two (x, y) points, got {start_point!r} and {end_point!r}")
        self.predecessor, self.ancestor, self.color = predecessor, ancestor, color
        self.vector = self._end_point - self._start_point
        self._length = np.linalg.norm(self.vector)
        self.angle = np.arctan2(self.vector[1], self.vector[0])

    @property
    def length(self):
        return self._length

    @property
    def start_point(self):
        return self._start_point

    @property
    def end_point(self):
        return self._end_point

    def get_position_at_distance(self, distance):
        """(x, y) at `distance` from the start, the distance clamped to [0, length]."""
        distance = max(0, min(distance, self.length))
        return self.start_point + (distance / self.length) * self.vector

    def distance_to_end(self, current_position):
        """Distance from a position on the edge to its end: the projection on the edge's direction, at least 0."""
        return max(0, np.dot(self.end_point - current_position, self.vector / self.length))

    def __repr__(self):
        return (f"Edge(start={tuple(self.start_point)}, end={tuple(self.end_point)}, length={self.length:.2f}, "
                f"angle={np.degrees(self.angle):.2f}°)")


class PackedGeometries(dict):
    """The arrays of pack_geometries: a dict that also keeps their copies on the devices they were used on."""

    def on(self, device):
        """(verts, lengths, vert_offsets, totals) as tensors on `device`, uploaded once.  The arrays are not meant to change
        after the first upload."""
        cache = self.__dict__.setdefault("_device", {})
        key = str(device)
        if key not in cache:
            cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(self[k])).to(device)
                               for k in ("verts", "lengths", "vert_offsets", "totals"))
        return cache[key]

    def max_edges(self):
        return int(np.diff(self["vert_offsets"]).max()) - 1


def pack_geometries(geometries) -> dict:
    """Geometries (a Geometry, a sequence of them, or sequences of Edge) -> the packed arrays every mapping here takes:
    verts [V, 2] float64 (each edge's start point and the last edge's end point), vert_offsets [G + 1] int32, lengths [V]
    float64 (lengths[v] = np.linalg.norm(verts[v + 1] - verts[v]) as Edge computes it; the last slot of a geometry is 0 and
    unused), totals [G] float64 (the ascending sequential sum, as Geometry computes it).  ValueError for an empty geometry, a
    non-finite vertex, a zero-length edge (the mapping divides by it) and edges that do not connect (np.allclose, as in the
    reference; where two ends agree only to that tolerance the packed vertex is the later edge's start)."""
    if isinstance(geometries, Geometry):
        geometries = [geometries]
    verts, lengths, offsets, totals = [], [], [0], []
    for g, geom in enumerate(geometries):
        edges = list(geom.edges if isinstance(geom, Geometry) else geom)
        if not edges:
            raise ValueError(f"geometry {g} is empty")
        total = None
        for i, e in enumerate(edges):
            if not (np.isfinite(e.start_point).all() and np.isfinite(e.end_point).all()):
                raise ValueError(f"geometry {g}, edge {i}: non-finite vertex {tuple(e.start_point)} -> {tuple(e.end_point)}")
            if not e.length > 0:
                raise ValueError(f"geometry {g}, edge {i}: zero length at {tuple(e.start_point)}")
            if i and not np.allclose(edges[i - 1].end_point, e.start_point):
                raise ValueError(f"Edges don't connect properly at index {i - 1}. "
                                 f"End point of edge {i - 1}: {tuple(edges[i - 1].end_point)}, "
                                 f"Start point of edge {i}: {tuple(e.start_point)}")
            verts.append(e.start_point)
            lengths.append(e.length)
            total = e.length if total is None else total + e.length
        verts.append(edges[-1].end_point)
        lengths.append(0.0)
        offsets.append(len(verts))
        totals.append(total)
    if not totals:
        raise ValueError("no geometry")
    return PackedGeometries(verts=np.array(verts, dtype=np.float64).reshape(-1, 2), vert_offsets=np.array(offsets, dtype=np.int32),
                            lengths=np.array(lengths, dtype=np.float64), totals=np.array(totals, dtype=np.float64))


def _map_host(disp, s0, geom_of, packed, mode):
    """The arithmetic of csrc/confine.hip in numpy (include/mivit_hip.h, mivit_map_displacements): vectorised over particles,
    sequential over steps and over edges.  disp [N, T], s0 [N] float64, geom_of [N] in [0, G), mode 0 (clamp) or 1 (reflect)
    -> pos [N, T, 2] float64, arc [N, T] float64, edge [N, T] int32."""
    N, T = disp.shape
    L = packed["totals"][geom_of]
    P = 2.0 * L

    def clamp(m, hi):
        m = np.where(hi < m, hi, m)
        return np.where(m > 0, m, 0.0)

    def bound(m):
        if mode == 1:
            m = np.fmod(m, P)
            m = np.where(m < 0, m + P, m)
            m = np.where(m > L, P - m, m)
        return clamp(m, L)

    arc = np.empty((N, T), np.float64)
    pos = np.empty((N, T, 2), np.float64)
    edge = np.empty((N, T), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = bound(np.asarray(s0, np.float64))
        for t in range(T):
            s = bound(s + disp[:, t])
            arc[:, t] = s
        for g in np.unique(geom_of):
            rows = np.nonzero(geom_of == g)[0]
            v0, v1 = int(packed["vert_offsets"][g]), int(packed["vert_offsets"][g + 1])
            verts, lens, E = packed["verts"][v0:v1], packed["lengths"][v0:v1 - 1], v1 - v0 - 1
            rem = arc[rows]
            open_ = np.ones(rem.shape, bool)
            p = np.broadcast_to(verts[E], rem.shape + (2,)).copy()           # no edge found: the last vertex, the last edge
            ed = np.full(rem.shape, E - 1, np.int32)
            for e in range(E):
                hit = open_ & (rem <= lens[e])                               # at a vertex the earlier edge wins
                f = clamp(rem[hit], lens[e]) / lens[e]
                p[hit] = verts[e] + f[:, None] * (verts[e + 1] - verts[e])
                ed[hit] = e
                open_ &= ~hit
                if not open_.any():
                    break
                rem = np.where(open_, rem - lens[e], rem)
            pos[rows], edge[rows] = p, ed
    return pos, arc, edge


def map_displacements(disp, s0, geometries, geom_of=None, boundary="clamp", return_arc_edge=False):
    """Displacements along filaments -> positions.  disp [N, T], s0 a number or [N] start arcs, geometries a Geometry, a
    sequence of G of them or a dict from pack_geometries, geom_of [N] integers in [0, G) (default arange(N) % G) -> pos
    [N, T, 2] float64 in the vertices' component order, and with return_arc_edge also arc [N, T] float64 (the arc after each
    step) and edge [N, T] int32 (the edge's index within its geometry).  boundary "clamp" is the reference (the arc is clamped
    to [0, total] at the start and after every step), "reflect" folds it back at both ends, per step.  A CUDA tensor goes to the
    kernel (ops.map_displacements: one launch, at most ops.GEOM_MAX_EDGES edges per geometry) and comes back as CUDA tensors;
    a CPU tensor or an array goes to the numpy restatement, which is bitwise the same arithmetic, and comes back in kind."""
    if boundary not in BOUNDARIES:
        raise ValueError(f"boundary must be one of {BOUNDARIES}, got {boundary!r}")
    mode = BOUNDARIES.index(boundary)
    packed = geometries if isinstance(geometries, dict) else pack_geometries(geometries)
    if not isinstance(packed, PackedGeometries):
        packed = PackedGeometries(packed)
    G = len(packed["totals"])
    is_t = torch.is_tensor(disp)
    if len(disp.shape) != 2:
        raise ValueError(f"disp must be [N, T], got {tuple(disp.shape)}")
    N = int(disp.shape[0])
    on_gpu = is_t and disp.device.type == "cuda"
    if on_gpu and torch.is_tensor(s0) and s0.device == disp.device:          # a start drawn on the GPU stays there
        start = s0.detach().double().reshape(-1)
        if start.numel() == 1 and N != 1:
            start = start.expand(N)
        n_start = start.numel()
    else:
        start = s0.detach().cpu().numpy() if torch.is_tensor(s0) else s0
        start = np.array(start, dtype=np.float64).reshape(-1)
        if start.size == 1 and N != 1:
            start = np.repeat(start, N)
        n_start = start.size
    if n_start != N:
        raise ValueError(f"s0 must be a number or hold one start per particle ({N}), got {n_start}")
    if geom_of is None:
        gof = np.arange(N, dtype=np.int64) % G
    else:
        gof = geom_of.detach().cpu().numpy() if torch.is_tensor(geom_of) else np.asarray(geom_of)
        if gof.dtype.kind not in "iu" or gof.shape != (N,):
            raise ValueError(f"geom_of must hold one integer per particle ({N}), got {gof.dtype} {gof.shape}")
        if N and (gof.min() < 0 or gof.max() >= G):
            raise ValueError(f"geom_of must lie in [0, {G})")
    if on_gpu:
        from .. import ops
        if packed.max_edges() > ops.GEOM_MAX_EDGES:
            raise ValueError(f"a geometry has {packed.max_edges()} edges, the kernel's limit is {ops.GEOM_MAX_EDGES} "
                             f"(ops.GEOM_MAX_EDGES)")
        dev = disp.device
        if not torch.is_tensor(start):
            start = torch.from_numpy(start).to(dev)
        # everything was checked here on the host copies: no second validation, no read-back from the device
        pos, arc, edge = ops._map_displacements_checked(disp.detach().double().contiguous(), start.contiguous(),
                                                        torch.from_numpy(gof.astype(np.int32)).to(dev), *packed.on(dev), mode)
    else:
        d = disp.detach().double().numpy() if is_t else np.asarray(disp, dtype=np.float64)
        pos, arc, edge = _map_host(d, start, gof, packed, mode)
        if is_t:
            pos, arc, edge = torch.from_numpy(pos), torch.from_numpy(arc), torch.from_numpy(edge)
    return (pos, arc, edge) if return_arc_edge else pos


class Geometry:
    """A chain of connected edges.  total_length is the ascending sum of the edge lengths, min_x .. max_y the bounding box;
    every edge gets its predecessor and ancestor.  Edges that do not connect (np.allclose) raise the reference's ValueError;
    unlike the reference an empty chain, a zero-length edge and a non-finite vertex raise one too (pack_geometries)."""

    def __init__(self, edges):
        self.edges = list(edges)
        self._packed = pack_geometries([self.edges])
        for cur, nxt in zip(self.edges[:-1], self.edges[1:]):
            nxt.predecessor, cur.ancestor = cur, nxt
        self.total_length = self._packed["totals"][0]
        pts = self._packed["verts"]
        self.min_x, self.max_x = np.min(pts[:, 0]), np.max(pts[:, 0])
        self.min_y, self.max_y = np.min(pts[:, 1]), np.max(pts[:, 1])

    def get_edge_at_position(self, position):
        """The first edge that holds `position` (within 1e-10 of its line, projection inside the edge), or None."""
        for edge in self.edges:
            rel = position - edge.start_point
            direction = edge.vector / edge.length
            along = np.dot(rel, direction)
            if 0 <= along <= edge.length and np.linalg.norm(rel - along * direction) < 1e-10:
                return edge
        return None

    def get_edge_at_length(self, distance):
        """(edge, distance along it) at `distance` from the start of the chain by sequential subtraction of the edge lengths; the
        earlier edge at a vertex; (None, 0) for a negative distance or one past the end."""
        if distance < 0:
            return None, 0
        remaining = distance
        for edge in self.edges:
            if remaining <= edge.length:
                return edge, remaining
            remaining -= edge.length
        return None, 0

    def draw(self, ax=None, edge_color="blue", vertex_color="red", edge_width=1.5, vertex_size=20, show_vertices=False,
             show_labels=False):
        """Draw the chain with matplotlib (each edge in its own color, as in the reference) and return the axis."""
        import matplotlib.pyplot as plt
        if ax is None:
            _, ax = plt.subplots(figsize=(10, 8))
        for i, edge in enumerate(self.edges):
            ax.plot([edge.start_point[0], edge.end_point[0]], [edge.start_point[1], edge.end_point[1]], color=edge.color,
                    linewidth=edge_width)
            if show_labels:
                mid = edge.get_position_at_distance(edge.length / 2)
                ax.text(mid[0], mid[1], f"{i}", ha="center", va="center", backgroundcolor="white")
        if show_vertices:
            pts = self._packed["verts"]
            ax.scatter(pts[:, 0], pts[:, 1], color=vertex_color, s=vertex_size, zorder=10)
        pad = 0.1 * max(self.max_x - self.min_x, self.max_y - self.min_y)
        ax.set_xlim(self.min_x - pad, self.max_x + pad)
        ax.set_ylim(self.min_y - pad, self.max_y + pad)
        ax.set_aspect("equal")
        ax.set_xlabel("X")
        ax.set_ylabel("Y")
        ax.set_title("Mitochondria Geometry")
        return ax

    def __repr__(self):
        return f"Geometry(edges={len(self.edges)}, total_length={self.total_length:.2f})"

    def map_displacements(self, displacements, initial_distance=0.0, boundary="clamp"):
        """1-D displacements along the chain -> 2-D positions.  A 1-D array of T displacements gives the reference's [T, 2]
        array; [N, T] with initial_distance a number or N values is the batched form, [N, T, 2].  See map_displacements."""
        d = displacements if torch.is_tensor(displacements) else np.asarray(displacements, dtype=np.float64)
        if d.ndim == 1:
            return map_displacements(d.reshape(1, -1), initial_distance, self._packed, boundary=boundary)[0]
        return map_displacements(d, initial_distance, self._packed, boundary=boundary)


def draw_trajectory(positions, ax=None, marker_size=10, connect_points=False, line_width=1, colormap="autumn", alpha=0.8,
                    show_label=False):
    """Scatter a trajectory [T, 2] with a color gradient over time (optionally joined by a line, optionally with a colorbar)
    and return the axis."""
    import matplotlib.pyplot as plt
    if ax is None:
        _, ax = plt.subplots(figsize=(10, 8))
    positions = np.asarray(positions)
    n = len(positions)
    if connect_points and n > 1:
        ax.plot(positions[:, 0], positions[:, 1], color="gray", linewidth=line_width, alpha=alpha, zorder=5)
    ax.scatter(positions[:, 0], positions[:, 1], c=np.linspace(0, 1, n), cmap=colormap, s=marker_size, alpha=alpha, zorder=10)
    if n > 1 and show_label:
        sm = plt.cm.ScalarMappable(cmap=plt.get_cmap(colormap), norm=plt.Normalize(0, n - 1))
        sm.set_array([])
        plt.colorbar(sm, ax=ax).set_label("Time progression")
    return ax


def disp_fbm(alpha, D, T, deltaT=1, generator=None, device="cpu"):
    """T displacements of fractional Brownian motion with <x^2(t)> = 2 D t^alpha, <x^2(1)> = 2 D deltaT:
    fractional_gaussian_noise(z [1, T, 1], alpha) * sqrt(2 D deltaT) with z = randn from `generator` on `device`.  EXACT (the
    Cholesky factor applied to z, helpers/generation) where the reference draws from the Davies-Harte method of the `fbm`
    package, which is exact in distribution too: the law is the same, the numbers are not.  Returns a float64 array [T] on the
    CPU, a CUDA tensor [T] on the GPU, where T <= ops.FGN_MAX_T."""
    from .generation import fractional_gaussian_noise
    dev = torch.device(device)
    z = torch.randn(1, int(T), 1, dtype=torch.float64, generator=generator, device=dev)
    out = (fractional_gaussian_noise(z, alpha) * math.sqrt(2 * D * deltaT)).reshape(int(T))
    return out if dev.type == "cuda" else out.numpy()


def cristae_geometry(n_cristae, spacing, depth, width, lead=0.0, origin=(0, 0), entry=0.0, tail=None):
    """A serpentine of cristae: a base line along +x from which n_cristae rectangular fingers rise `depth` high (+y) and
    `width` wide, `spacing` of base line between two fingers; depth may be one number or n_cristae of them.  Vertex order, with
    origin = (x0, y0): [from (x0, y0 + entry) down to the origin, if entry > 0], [lead along +x, if lead > 0], then per finger up
    `depth`, across `width`, down `depth`, then `spacing` along +x before the next finger, and after the last finger [tail
    along +x, if tail > 0; tail defaults to lead].  3 n + (n - 1) + [entry > 0] + [lead > 0] + [tail > 0] edges, total length
    sum(2 depth + width) + (n - 1) spacing + entry + lead + tail.  The ten-edge example of the reference's notebook is
    cristae_geometry(2, 100, (200, 250), 30, lead=100, entry=300, tail=90)."""
    n = int(n_cristae)
    depths = np.broadcast_to(np.asarray(depth, dtype=np.float64), (n,)) if n >= 1 else None
    tail = lead if tail is None else tail
    if n < 1 or not (spacing > 0 and width > 0 and lead >= 0 and entry >= 0 and tail >= 0 and (depths > 0).all()):
        raise ValueError(f"need n_cristae >= 1, spacing, depth, width > 0 and lead, entry, tail >= 0, got {n_cristae}, {spacing}, "
                         f"{depth}, {width}, {lead}, {entry}, {tail}")
    x, y = float(origin[0]), float(origin[1])
    pts = [(x, y + entry), (x, y)] if entry > 0 else [(x, y)]
    if lead > 0:
        x += lead
        pts.append((x, y))
    for i in range(n):
        pts.append((x, y + depths[i]))
        x += width
        pts.append((x, y + depths[i]))
        pts.append((x, y))
        if i < n - 1:
            x += spacing
            pts.append((x, y))
    if tail > 0:
        pts.append((x + tail, y))
    fingers = pts[2:] if entry > 0 else pts[1:]                               # the entry edge is drawn like the base line
    return Geometry([Edge(a, b, color="cyan" if b in fingers and (a[1] != y or b[1] != y) else "blue")
                     for a, b in zip(pts[:-1], pts[1:])])

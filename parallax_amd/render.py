"""Render export: env.draw(painter) without host callbacks.

The reference draws from inside jit through jax.debug.callback into a
pygame PyPainter (cotix/_viz.py:6-75): RoboCupEnv.draw (cotix/_robocup.py:
140-150) fills every body with its colour and outlines it with its edge
colour; LunarLander.draw (cotix/_lunar_lander.py:220-225) draws every body
with the shapes' default colours plus two red lines.  Here the per-env
geometry of those draws is one device kernel (cotix_render: every part
transformed by its body -- circles as (cx, cy, r), AABB and polygon edges in
get_edges order) and the static part -- which primitive, which colour, in
which order -- is a command list built once per scenario.  replay() issues the
reference's exact Painter call sequence for one env from that table, so any
object with draw_circle / draw_line / next (a PyPainter included) works.

pixels() goes the last step to an image observation: every env's filled
bodies rasterized by one device kernel (cotix_rasterize, DESIGN.md section
16) into a uint8 tensor of body ids or planar RGB -- filled bodies only: no
outlines, none of LunarLander's two red lines, no anti-aliasing.

rays() is the low-dimensional observation of the same geometry: a fan of rays
cast from a RaySensor in every env by one device kernel (cotix_raycast,
DESIGN.md section 17), each reporting the distance to the nearest boundary
crossing of a part and that part's body.  rays_backward() is its
vector-Jacobian product with respect to every body's pose and every geometry
word (cotix_raycast_backward) and differentiable_rays()
the torch.autograd surface over the two.
"""
import math

import torch

from . import _ffi
from .shapes import AABB, AbstractPolygon, Circle

# default colours of the shapes' draw() (cotix/_convex_shapes.py:43,119,189)
DEFAULT_COLOR = {"circle": (128, 128, 128), "aabb": (128, 128, 128), "polygon": (255, 255, 255)}


def _kind(part):
    if isinstance(part, Circle):
        return "circle"
    if isinstance(part, AABB):
        return "aabb"
    if isinstance(part, AbstractPolygon):
        return "polygon"
    raise TypeError("unknown part type %r" % type(part))


def part_layout(bodies):
    """[(kind, first primitive, primitive count)] per part, parts in scene
    order (the kernel's layout: circle 1, AABB 4, polygon n primitives)."""
    out, off = [], 0
    for b in bodies:
        for p in b.shape.parts:
            k = _kind(p)
            n = 1 if k == "circle" else (4 if k == "aabb" else p.vertices.shape[-2])
            out.append((k, off, n))
            off += n
    return out


def render(world, dyn=None):
    """f32 [B, n_prims, 4] on the world's device: the transformed geometry of
    every drawn primitive of every env (cotix_render)."""
    d = world.dyn if dyn is None else dyn
    n = _ffi.lib.cotix_render_count(world.scene.handle)
    if n < 0:
        _ffi.check(n, "cotix_render_count")
    layout = part_layout(world.bodies)
    if layout and layout[-1][1] + layout[-1][2] != n:
        raise RuntimeError("render layout mismatch with the library")
    out = torch.empty(world.B, n, 4, dtype=torch.float32, device=world.device)
    _ffi.check(_ffi.lib.cotix_render(world.scene.handle, _ffi.ptr(d), _ffi.ptr(world.geom), world.geom_stride,
                                     world.B, _ffi.ptr(out), _ffi.stream_ptr(world.device)), "cotix_render")
    return out


def _shape_cmds(layout, parts_of_body, color):
    """UniversalShape.draw(painter, [color]) -> part.transform(T).draw(...)."""
    cmds = []
    for p in parts_of_body:
        k, off, n = layout[p]
        c = DEFAULT_COLOR[k] if color is None else color
        if k == "circle":
            cmds.append(("circle", off, c))
        else:  # AABB.draw and Polygon.draw both draw their edges
            cmds.extend(("line", off + q, c) for q in range(n))
    return cmds


def _edge_cmds(layout, parts_of_body, color):
    """UniversalShape.drawEdges(painter, color=...)."""
    cmds = []
    for p in parts_of_body:
        k, off, n = layout[p]
        if k == "circle":
            raise NotImplementedError("Circle.drawEdges (cotix/_convex_shapes.py:46-47)")
        cmds.extend(("line", off + q, color) for q in range(n))
    return cmds


def _parts_by_body(bodies):
    out, p = [[] for _ in bodies], 0
    for i, b in enumerate(bodies):
        for _ in b.shape.parts:
            out[i].append(p)
            p += 1
    return out


def commands_bodies(bodies, colors=None, edge_colors=None, extra_lines=()):
    """The draw command list of `for body: shape.draw(color); shape.drawEdges(edge_color)`
    then static lines.  colors / edge_colors: per body, None = default / no edge pass."""
    layout = part_layout(bodies)
    pb = _parts_by_body(bodies)
    cmds = []
    for i in range(len(bodies)):
        cmds.extend(_shape_cmds(layout, pb[i], None if colors is None else colors[i]))
        if edge_colors is not None and edge_colors[i] is not None:
            cmds.extend(_edge_cmds(layout, pb[i], edge_colors[i]))
    for (a, b, c) in extra_lines:
        cmds.append(("static_line", (a, b), c))
    return cmds


def replay(painter, cmds, prims, env=0):
    """Issue the Painter calls of one env; prims: the render() output (any
    device; moved to the host here), then painter.next() as the reference's
    draw() ends with."""
    g = prims[env].detach().to("cpu").tolist() if isinstance(prims, torch.Tensor) else prims[env]
    for op, ref, color in cmds:
        if op == "circle":
            x, y, r, _ = g[ref]
            painter.draw_circle((x, y), r, color)
        elif op == "line":
            x0, y0, x1, y1 = g[ref]
            painter.draw_line((x0, y0), (x1, y1), color)
        else:
            painter.draw_line(ref[0], ref[1], color)
    painter.next()


class Camera:
    """The window of pixels(): `center` +- `half_extent` in world units (the
    default is PyPainter's 16 x 12 window around the origin), or, with
    follow_body, in the frame of that body of every env: shifted by its
    position and, with follow_angle, turned by its angle (an egocentric
    view).  Immutable."""

    __slots__ = ("center", "half_extent", "follow_body", "follow_angle")

    def __init__(self, center=(0.0, 0.0), half_extent=(8.0, 6.0), follow_body=None, follow_angle=False):
        set_ = object.__setattr__
        set_(self, "center", (float(center[0]), float(center[1])))
        set_(self, "half_extent", (float(half_extent[0]), float(half_extent[1])))
        set_(self, "follow_body", None if follow_body is None else int(follow_body))
        set_(self, "follow_angle", bool(follow_angle))

    def __setattr__(self, name, value):
        raise AttributeError("Camera is immutable: build a new one")

    __delattr__ = __setattr__

    def __repr__(self):
        return "Camera(center=%r, half_extent=%r, follow_body=%r, follow_angle=%r)" % (
            self.center, self.half_extent, self.follow_body, self.follow_angle)

    def c_struct(self):
        """struct cotix_camera (include/cotix_amd.h)."""
        return _ffi.CotixCamera(self.center[0], self.center[1], self.half_extent[0], self.half_extent[1],
                                -1 if self.follow_body is None else self.follow_body, 1 if self.follow_angle else 0)


def palette_bytes(palette, n_bodies):
    """A palette (n_bodies + 1 RGB triples, entry 0 the background) as the
    3 * (n_bodies + 1) bytes cotix_rasterize reads."""
    rows = [tuple(int(c) for c in rgb) for rgb in palette]
    if len(rows) != n_bodies + 1 or any(len(r) != 3 or min(r) < 0 or max(r) > 255 for r in rows):
        raise ValueError("palette must be %d RGB triples of bytes (the background, then one per body)"
                         % (n_bodies + 1))
    return bytes(c for r in rows for c in r)


def pixels(world, width, height, camera=None, palette=None, dyn=None, out=None):
    """Image observations of every env (cotix_rasterize): torch.uint8 on the
    world's device, [B, H, W] body ids (0: background, 1 + b: body b, the
    last body in scene order that covers the pixel) or, with a palette,
    [B, 3, H, W] planar RGB.  camera: a Camera (default: PyPainter's window);
    dyn: a state tensor in world.dyn's layout (default world.dyn); out: a
    tensor of the result's shape to write into (no allocation per call)."""
    width, height = int(width), int(height)
    nb = len(world.bodies)
    pal = None if palette is None else palette_bytes(palette, nb)
    shape = (world.B, height, width) if pal is None else (world.B, 3, height, width)
    d = world.dyn if dyn is None else dyn
    if tuple(d.shape) != tuple(world.dyn.shape) or d.dtype != torch.float32 or d.device != world.dyn.device:
        raise ValueError("dyn must be an f32 [n_bodies, 6, B] tensor on the world's device")
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=world.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != world.dyn.device \
            or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 %s tensor on the world's device" % list(shape))
    cam = (Camera() if camera is None else camera).c_struct()
    _ffi.check(_ffi.lib.cotix_rasterize(world.scene.handle, _ffi.ptr(d), _ffi.ptr(world.geom), world.geom_stride,
                                        world.B, cam, width, height, 1 if pal is None else 3, pal,
                                        _ffi.ptr(out), _ffi.stream_ptr(world.device)), "cotix_rasterize")
    return out


class RaySensor:
    """The range sensor of rays(): mounted at `offset` in the frame of `body`
    of every env (shifted by its position and, with follow_angle, turned by
    its angle), or, without a body, fixed at `offset` in the world.  Bodies in
    `ignore` are invisible to the rays; by default that is the sensor's own
    body, whose boundary every ray would otherwise cross on its way out.
    Immutable."""

    __slots__ = ("body", "offset", "follow_angle", "max_range", "ignore")

    def __init__(self, body=None, offset=(0.0, 0.0), follow_angle=False, max_range=10.0, ignore=None):
        set_ = object.__setattr__
        set_(self, "body", None if body is None else int(body))
        set_(self, "offset", (float(offset[0]), float(offset[1])))
        set_(self, "follow_angle", bool(follow_angle))
        set_(self, "max_range", float(max_range))
        if ignore is None:
            ignore = () if body is None else (body,)
        ignore = tuple(sorted({int(b) for b in ignore}))
        if any(b < 0 or b > 31 for b in ignore):
            raise ValueError("ignore holds body indices in [0, 32)")
        set_(self, "ignore", ignore)

    def __setattr__(self, name, value):
        raise AttributeError("RaySensor is immutable: build a new one")

    def __delattr__(self, name):
        raise AttributeError("RaySensor is immutable: build a new one")

    def __repr__(self):
        return "RaySensor(body=%r, offset=%r, follow_angle=%r, max_range=%r, ignore=%r)" % (
            self.body, self.offset, self.follow_angle, self.max_range, self.ignore)

    @staticmethod
    def fan(n, fov=2.0 * math.pi, start=None):
        """The direction table of n rays spread evenly over `fov` radians:
        ray k points at angle start + (k + 1/2) * fov / n, counter-clockwise
        from the x axis of the sensor's frame; start defaults to -fov / 2, a
        fan centred on that axis.  f32 [n, 2] on the host: cos and sin taken in
        float64, then rounded."""
        n = int(n)
        if n < 1:
            raise ValueError("a fan has at least one ray")
        start = -0.5 * fov if start is None else float(start)
        ang = start + (torch.arange(n, dtype=torch.float64) + 0.5) * (float(fov) / n)
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).to(torch.float32)

    def c_struct(self):
        """struct cotix_ray_sensor (include/cotix_amd.h)."""
        mask = 0
        for b in self.ignore:
            mask |= 1 << b
        return _ffi.CotixRaySensor(-1 if self.body is None else self.body, 1 if self.follow_angle else 0,
                                   self.offset[0], self.offset[1], self.max_range, mask)


def rays(world, sensor, dirs, dyn=None, out=None, hit_out=None):
    """Range readings of every env (cotix_raycast): (dist, hit), f32 and uint8
    [B, n_rays] on the world's device.  dist is the distance, in units of the
    direction's length, to the nearest boundary crossing of a visible part
    along each ray, hit 1 + that part's body; sensor.max_range and 0 where
    there is none.  These are crossings, not entries: a ray that starts inside
    a shape reports where it leaves it.  dirs: f32 [n_rays, 2] on the world's
    device (RaySensor.fan(n).to(device)); dyn: a state tensor in world.dyn's
    layout (default world.dyn); out: a tensor of dist's shape to write into (no
    allocation per call); hit_out: the tensor the ids are written into --
    without one no ids are written and hit is None."""
    dev = world.dyn.device
    if not isinstance(sensor, RaySensor):
        raise TypeError("sensor must be a RaySensor")
    if not torch.is_tensor(dirs) or dirs.dim() != 2 or dirs.shape[1] != 2 or dirs.dtype != torch.float32 \
            or dirs.device != dev or not dirs.is_contiguous():
        raise ValueError("dirs must be a contiguous f32 [n_rays, 2] tensor on the world's device")
    shape = (world.B, int(dirs.shape[0]))
    d = world.dyn if dyn is None else dyn
    if tuple(d.shape) != tuple(world.dyn.shape) or d.dtype != torch.float32 or d.device != dev:
        raise ValueError("dyn must be an f32 [n_bodies, 6, B] tensor on the world's device")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous f32 %s tensor on the world's device" % list(shape))
    if hit_out is not None and (tuple(hit_out.shape) != shape or hit_out.dtype != torch.uint8 or hit_out.device != dev
                                or not hit_out.is_contiguous()):
        raise ValueError("hit_out must be a contiguous uint8 %s tensor on the world's device" % list(shape))
    _ffi.check(_ffi.lib.cotix_raycast(world.scene.handle, _ffi.ptr(d), _ffi.ptr(world.geom), world.geom_stride,
                                      world.B, sensor.c_struct(), _ffi.ptr(dirs), shape[1], _ffi.ptr(out),
                                      _ffi.ptr(hit_out), _ffi.stream_ptr(world.device)), "cotix_raycast")
    return out, hit_out


def _check_dirs_dyn(world, sensor, dirs, dyn):
    dev = world.dyn.device
    if not isinstance(sensor, RaySensor):
        raise TypeError("sensor must be a RaySensor")
    if not torch.is_tensor(dirs) or dirs.dim() != 2 or dirs.shape[1] != 2 or dirs.dtype != torch.float32 \
            or dirs.device != dev or not dirs.is_contiguous():
        raise ValueError("dirs must be a contiguous f32 [n_rays, 2] tensor on the world's device")
    d = world.dyn if dyn is None else dyn
    if not torch.is_tensor(d) or tuple(d.shape) != tuple(world.dyn.shape) or d.dtype != torch.float32 \
            or d.device != dev:
        raise ValueError("dyn must be an f32 [n_bodies, 6, B] tensor on the world's device")
    return d


def rays_backward(world, sensor, dirs, grad_dist, dyn=None, want_dyn=True, want_geom=False):
    """The vector-Jacobian product of rays()' dist with the cotangent
    grad_dist (cotix_raycast_backward): (g_dyn, g_geom).
    g_dyn, f32 [n_bodies, 6, B], holds sum_k grad_dist[env, k] * d dist[env, k]
    / d (px, py, angle) of every body in rows 0, 1 and 4 (the velocity rows are
    0); g_geom, f32 [GW, B], the same sum for every word of World.geometry() --
    on shared geometry column `env` is that env's derivative with respect to
    the shared word (sum over envs for a batch objective).  The one not wanted
    is None.  The rays are cast again from `dyn` (default world.dyn) and the
    world's geometry: the derivative is that of the crossing each ray reports,
    held fixed; a ray that crosses nothing, and a ray whose grad_dist is 0,
    contribute nothing whatever else grad_dist holds.  grad_dist: a contiguous
    f32 [B, n_rays] tensor on the world's device."""
    dev = world.dyn.device
    d = _check_dirs_dyn(world, sensor, dirs, dyn)
    shape = (world.B, int(dirs.shape[0]))
    if not torch.is_tensor(grad_dist) or tuple(grad_dist.shape) != shape or grad_dist.dtype != torch.float32 \
            or grad_dist.device != dev or not grad_dist.is_contiguous():
        raise ValueError("grad_dist must be a contiguous f32 %s tensor on the world's device" % list(shape))
    if not want_dyn and not want_geom:
        raise ValueError("rays_backward: want_dyn and want_geom are both False")
    gd = torch.empty(tuple(world.dyn.shape), dtype=torch.float32, device=dev) if want_dyn else None
    gg = torch.empty(world.scene.geom_part_words, world.B, dtype=torch.float32, device=dev) if want_geom else None
    _ffi.check(_ffi.lib.cotix_raycast_backward(
        world.scene.handle, _ffi.ptr(d), _ffi.ptr(world.geom), world.geom_stride, world.B,
        sensor.c_struct(), _ffi.ptr(dirs), shape[1], _ffi.ptr(grad_dist), _ffi.ptr(gd), _ffi.ptr(gg),
        _ffi.stream_ptr(world.device)), "cotix_raycast_backward")
    return gd, gg


class _Rays(torch.autograd.Function):
    """rays() with the state and, optionally, the geometry as differentiable inputs."""

    @staticmethod
    def forward(ctx, dyn, geometry, world, sensor, dirs, hit_out):
        if geometry is not None:
            world.geometry().copy_(geometry.detach())
        # a private copy: a later step does not move what the rays were cast from
        state = dyn.detach().clone(memory_format=torch.contiguous_format)
        dist, _ = rays(world, sensor, dirs, dyn=state, hit_out=hit_out)
        ctx.world, ctx.sensor, ctx.dirs, ctx.state = world, sensor, dirs, state
        ctx.geom_version = world.geom._version
        return dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dist):
        w = ctx.world
        if w.geom._version != ctx.geom_version:
            raise RuntimeError("the world's geometry changed between differentiable_rays() and backward()")
        want_d, want_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not want_d and not want_g:
            return None, None, None, None, None, None
        gd, gg = rays_backward(w, ctx.sensor, ctx.dirs, g_dist.to(torch.float32).contiguous(), dyn=ctx.state,
                               want_dyn=want_d, want_geom=want_g)
        if want_g:
            gg = gg.T.contiguous() if w.geom.dim() == 2 else gg.sum(dim=1)
        return gd, gg, None, None, None, None


def differentiable_rays(world, sensor, dirs, dyn=None, geometry=None, hit_out=None):
    """rays()' dist, f32 [B, n_rays], differentiable through torch.autograd with
    respect to `dyn` and `geometry` (the backward is cotix_raycast_backward:
    rays_backward above states what the derivative is).

    dyn: an f32 [n_bodies, 6, B] tensor on the world's device, which may
    require grad (default: world.dyn, no gradient); its gradient has its shape,
    with zeros in the velocity rows.  geometry: as rollout(geometry=): a float32
    tensor of World.geometry()'s shape on the world's device, copied into
    ``world.geom`` before the rays are cast; its gradient is [B, GW] on per-env
    rows and the sum over the envs on shared geometry.  hit_out: as rays().

    The forward keeps a copy of the state it cast from, so stepping the world
    before backward() changes nothing; writing the world's geometry in between
    raises RuntimeError.  dirs, the sensor's offset and max_range are not
    differentiated, and the backward is not differentiable again."""
    d = _check_dirs_dyn(world, sensor, dirs, dyn)
    if geometry is not None:
        have = world.geometry()
        if not torch.is_tensor(geometry) or tuple(geometry.shape) != tuple(have.shape):
            raise ValueError("geometry must be %s for this world, got %s" % (
                tuple(have.shape), tuple(geometry.shape) if torch.is_tensor(geometry) else type(geometry)))
        if geometry.dtype != torch.float32 or geometry.device != have.device:
            raise ValueError("geometry must be a float32 tensor on the world's device")
    return _Rays.apply(d, geometry, world, sensor, dirs, hit_out)


def default_palette(bodies, background=(0, 0, 0)):
    """The background, then DEFAULT_COLOR of each body's first part (what
    shape.draw(painter) without a colour paints)."""
    return [tuple(background)] + [DEFAULT_COLOR[_kind(b.shape.parts[0])] for b in bodies]


class RecordingPainter:
    """A Painter that records its calls (tests, headless use)."""

    def __init__(self):
        self.calls = []

    def draw_circle(self, center, radius, color):
        self.calls.append(("circle", tuple(center), radius, tuple(color)))

    def draw_line(self, start, end, color):
        self.calls.append(("line", tuple(start), tuple(end), tuple(color)))

    def draw_polygon(self, vertices, color):
        self.calls.append(("polygon", [tuple(v) for v in vertices], tuple(color)))

    def next(self):
        self.calls.append(("next",))

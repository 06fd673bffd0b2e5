"""Restatement in differentiable torch of what csrc/pvg.hip and csrc/envlight.hip compute: the vibration transform of Periodic
Vibration Gaussians, the cube-map sampler and the sky blend.  Run on float64 tensors it is the oracle of tests/test_pvg_gpu.py; run on
float32 tensors it is "the same formulation in fp32 torch" from whose error against the oracle the tests derive their bounds.

The motion part is the reference model's getters written out.  The cube-map part is written from the definition in
include/gspl_hip.h section 17 (face selection with its ties, s / t, the four taps, the fold over an edge, the dropped corner tap with
renormalisation); it is not translated from any package.

Also here: the seeded case builders, and a fake PVG model with the getters the renderer calls."""
import math
import types

import torch

F32_EPS = 2.0 ** -24                 # unit round-off of float32
MIN_BOUND = 8 * F32_EPS              # no bound derived from the fp32-torch error goes below this
# A float32 marginal below the smallest normal number (2^-126) may carry a single significant bit or be flushed to zero: its absolute
# error is up to 2^-126.  The "sum of the absolute terms" of everything that goes through the marginal is therefore formed with
# max(marginal, MARGINAL_FLOOR), the floor chosen so that MIN_BOUND times the floor is that absolute error.
MARGINAL_FLOOR = 2.0 ** -126 / MIN_BOUND


# ---- the vibration transform ----------------------------------------------------------------------------------------------------------
def motion(means, velocity, t, scale_t, opacities, time, time_offset, time_shift, cycle, velocity_decay):
    """(means_t, avg_velocity, opacity_t) in the dtype of the inputs; t, scale_t, opacities [N, 1].  periodic_vibration_gaussian.py:117-129
    and the renderer's lines 147-155, operation by operation."""
    a = 1 / cycle * math.pi * 2
    shift = 0.0 if time_shift is None else time_shift
    ts = time + time_offset - shift
    avg_velocity = velocity * torch.exp(-scale_t / cycle / 2 * velocity_decay)
    means_t = means + velocity * torch.sin((ts - t) * a) / a
    if time_shift is not None:
        means_t = means_t + avg_velocity * time_shift
    marginal = torch.exp(-0.5 * (t - ts) ** 2 / scale_t ** 2)
    return means_t, avg_velocity, opacities * marginal


def motion_term_sums(means, velocity, t, scale_t, opacities, time, time_offset, time_shift, cycle, velocity_decay, v_means_t, v_avg_velocity,
                     v_opacity_t):
    """The sum of the absolute values of the terms of every output element and of every gradient element, in float64: what the errors
    of tests/test_pvg_gpu.py are measured against.  -> (forward sums x3, gradient sums x5)."""
    d = lambda x: x.detach().double()
    means, velocity, t, scale_t, opacities, gm, gav, go = map(d, (means, velocity, t, scale_t, opacities, v_means_t, v_avg_velocity, v_opacity_t))
    a = 1 / cycle * math.pi * 2
    shift = 0.0 if time_shift is None else time_shift
    ts = float(time) + time_offset - shift
    e = torch.exp(-scale_t / cycle / 2 * velocity_decay)
    phase = (ts - t) * a
    s, co = torch.sin(phase).abs() / a, torch.cos(phase).abs()
    dt = (t - ts).abs()
    M = torch.exp(-0.5 * dt ** 2 / scale_t ** 2).clamp_min(MARGINAL_FLOOR)
    k = velocity_decay / (2 * cycle)
    fwd = ((means.abs() + velocity.abs() * s + velocity.abs() * e * abs(shift)), velocity.abs() * e, opacities.abs() * M)
    G = gav.abs() + abs(shift) * gm.abs()
    through_M = go.abs() * opacities.abs() * M
    grads = (gm.abs(), gm.abs() * s + G * e,
             (gm.abs() * velocity.abs()).sum(-1, keepdim=True) * co + through_M * dt / scale_t ** 2,
             (G * velocity.abs()).sum(-1, keepdim=True) * e * k + through_M * dt ** 2 / scale_t ** 3,
             go.abs() * M)
    return fwd, grads


def motion_case(n, seed=0):
    """Seeded rows of the default model (cycle 0.2, time_duration (-0.5, 0.5)): t over 1.2 durations, scale_t = exp(uniform(-6, 0)) so
    that some rows' marginal underflows, velocities of a few units per unit time.  float32, on the CPU."""
    g = torch.Generator().manual_seed(1000 + 17 * n + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    means = (r(n, 3) * 2 - 1) * 1.3
    velocity = torch.randn(n, 3, generator=g) * 2.0
    t = (r(n, 1) * 1.2 - 0.1) - 0.5
    scale_t = torch.exp(-6.0 * r(n, 1))
    opacities = torch.sigmoid(torch.randn(n, 1, generator=g))
    grads = (torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, 1, generator=g))
    return (means, velocity, t, scale_t, opacities), grads


# ---- the cube map -----------------------------------------------------------------------------------------------------------------------
def select_face(p):
    """p [..., 3] -> (face, sc, tc, ma): the major axis is x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z."""
    x, y, z = p.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    face = torch.where(is_x, torch.where(x >= 0, 0, 1), torch.where(is_y, torch.where(y >= 0, 2, 3), torch.where(z >= 0, 4, 5)))
    sc = torch.stack([-z, z, x, x, x, -x], dim=-1).gather(-1, face[..., None])[..., 0]
    tc = torch.stack([-y, -y, z, -z, -y, -y], dim=-1).gather(-1, face[..., None])[..., 0]
    ma = torch.stack([ax, ax, ay, ay, az, az], dim=-1).gather(-1, face[..., None])[..., 0]
    return face, sc, tc, ma


def face_point(face, u, v, m):
    """The point of face `face`'s extended plane at (u, v), its major coordinate of magnitude m: the inverse of select_face's table."""
    per_face = torch.stack([torch.stack([m, -v, -u], -1), torch.stack([-m, -v, u], -1), torch.stack([u, m, v], -1),
                            torch.stack([u, -m, -v], -1), torch.stack([u, -v, m], -1), torch.stack([-u, -v, -m], -1)], dim=-2)
    return per_face.gather(-2, face[..., None, None].expand(*face.shape, 1, 3))[..., 0, :]


def cube_taps(dirs, R):
    """dirs [M, 3] -> (texel [M, 4] int64 indices into base.reshape(6 R R, 3), weight [M, 4] in dirs' dtype).  A dropped corner tap and
    every tap of a zero or non-finite direction have weight 0 (and texel 0)."""
    dt = dirs.dtype
    bad = ~torch.isfinite(dirs).all(-1) | (dirs == 0).all(-1)
    safe = torch.where(bad[:, None], torch.tensor([1.0, 0.0, 0.0], dtype=dt, device=dirs.device), dirs)
    face, sc, tc, ma = select_face(safe)
    x = (sc / ma + 1) / 2 * R - 0.5
    y = (tc / ma + 1) / 2 * R - 0.5
    x0f, y0f = torch.floor(x), torch.floor(y)
    fx, fy = x - x0f, y - y0f
    x0, y0 = x0f.long().clamp(-1, R - 1), y0f.long().clamp(-1, R - 1)
    texels, weights = [], []
    has_corner = torch.zeros_like(bad)
    for k in range(4):
        xi, yi = x0 + (k & 1), y0 + (k >> 1)
        w = (fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy)
        out_x, out_y = (xi < 0) | (xi >= R), (yi < 0) | (yi >= R)
        corner, edge = out_x & out_y, out_x ^ out_y
        # the fold: the texel centre in [-1, 1] units; the overflowing coordinate becomes +-1, the former major coordinate 1 - 1/R;
        # the face and the nearest texel are selected again from the folded point
        u = (2 * xi.to(dt) + 1) * (1 / R) - 1
        v = (2 * yi.to(dt) + 1) * (1 / R) - 1
        u = torch.where(out_x, torch.where(xi < 0, -1.0, 1.0).to(dt), u)
        v = torch.where(out_y & ~out_x, torch.where(yi < 0, -1.0, 1.0).to(dt), v)
        f2, s2, t2, m2 = select_face(face_point(face, u, v, torch.full_like(u, 1 - 1 / R)))
        tx2 = torch.floor((s2 / m2 + 1) / 2 * R).long().clamp(0, R - 1)
        ty2 = torch.floor((t2 / m2 + 1) / 2 * R).long().clamp(0, R - 1)
        f = torch.where(edge, f2, face)
        tx = torch.where(edge, tx2, xi.clamp(0, R - 1))
        ty = torch.where(edge, ty2, yi.clamp(0, R - 1))
        dead = corner | bad
        has_corner |= corner & ~bad
        texels.append(torch.where(dead, 0, (f * R + ty) * R + tx))
        weights.append(torch.where(dead, torch.zeros_like(w), w))
    texel, weight = torch.stack(texels, -1), torch.stack(weights, -1)
    # a cube corner has no texel: its tap is dropped (an exact zero above) and the other three are divided by their sum
    kept = ((weight[:, 0] + weight[:, 1]) + weight[:, 2]) + weight[:, 3]
    inv = 1 / torch.where(has_corner, kept, torch.ones_like(kept))
    weight = torch.where(has_corner[:, None], weight * inv[:, None], weight)
    return texel, weight


def cubemap(base, dirs):
    """base [6, R, R, 3] sampled along dirs [M, 3] -> [M, 3]; differentiable in base."""
    texel, weight = cube_taps(dirs, base.shape[1])
    return (weight[..., None] * base.reshape(-1, 3)[texel]).sum(1)


def cubemap_grad_sums(R, dirs, v_out):
    """float64 [6 R R, 3]: per texel element, the sum of the absolute contributions weight |v_out| of every sample."""
    texel, weight = cube_taps(dirs.double(), R)
    sums = torch.zeros(6 * R * R, 3, dtype=torch.float64)
    sums.index_add_(0, texel.reshape(-1), (weight[..., None] * v_out.double().abs()[:, None, :]).reshape(-1, 3))
    return sums


def cubemap_directions(R, seed=0):
    """float32 [M, 3]: six axis-aligned fans that hit every face; points exactly on the 12 edges and 8 corners (the |x| = |y| ties)
    and within one texel of them; a zero and a NaN row; 1000 random rows."""
    g = torch.Generator().manual_seed(77 + R + seed)
    rows = []
    span = torch.linspace(-0.95, 0.95, 9)
    for axis in range(3):
        for sign in (1.0, -1.0):
            a, b = torch.meshgrid(span, span, indexing="ij")
            fan = torch.stack([a.reshape(-1), b.reshape(-1)], -1)
            fan = torch.cat([fan[:, :axis], torch.full((fan.shape[0], 1), sign), fan[:, axis:]], dim=1)
            rows.append(fan * (0.5 + torch.rand(fan.shape[0], 1, generator=g)))          # any length
    texel = 2.0 / R
    specials = []
    for a in (1.0, -1.0):
        for b in (1.0, -1.0):
            for free in (-0.6, 0.0, 0.37):
                for axis in range(3):          # the 12 edges: two coordinates tie at +-1, the third is free
                    p = [a, b]
                    p.insert(axis, free)
                    specials.append(p)
            for c in (1.0, -1.0):              # the 8 corners
                specials.append([a, b, c])
    specials = torch.tensor(specials)
    rows.append(specials)
    for scale in (0.25, 0.5, 0.999):           # within one texel of the edges and corners, on either side
        jitter = (torch.rand(specials.shape, generator=g) * 2 - 1) * texel * scale
        rows.append(specials + jitter)
    rows.append(torch.tensor([[0.0, 0.0, 0.0], [float("nan"), 1.0, 0.5]]))
    rows.append(torch.randn(1000, 3, generator=g))
    return torch.cat(rows).float()


# ---- the blend --------------------------------------------------------------------------------------------------------------------------
def pixel_directions(c2w_rotation, fx, fy, cx, cy, H, W, jitter=None):
    """[H, W, 3] in the dtype of c2w_rotation: the renderer's `get_world_directions` followed by EnvLight's axis swap."""
    dt = c2w_rotation.dtype
    v, u = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    ju, jv = (0.5, 0.5) if jitter is None else (jitter[0].to(dt), jitter[1].to(dt))
    d = torch.stack([(u - cx + ju) / fx, (v - cy + jv) / fy, torch.ones_like(u)], dim=-1)
    d = torch.nn.functional.normalize(d, dim=-1)
    w = d @ c2w_rotation.T
    return torch.stack([w[..., 0], w[..., 2], -w[..., 1]], dim=-1)


def blend(rgb, alpha, base, dirs):
    """rgb [3, H, W] + (1 - alpha [H, W]) sky, the sky sampled along dirs [H, W, 3]."""
    H, W = alpha.shape
    sky = cubemap(base, dirs.reshape(-1, 3)).reshape(H, W, 3).permute(2, 0, 1)
    return rgb + (1 - alpha)[None] * sky


def rotations():
    """Six camera-to-world rotations (float64): the identity, quarter turns that face other cube faces, and two oblique ones."""
    def axis_angle(axis, deg):
        axis = torch.tensor(axis, dtype=torch.float64)
        axis = axis / axis.norm()
        K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
        th = math.radians(deg)
        return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return [torch.eye(3, dtype=torch.float64), axis_angle([0, 1, 0], 90), axis_angle([1, 0, 0], -90), axis_angle([0, 1, 0], 180),
            axis_angle([1, 1, 0], 45), axis_angle([0.3, -1.0, 0.5], 131)]


# ---- a fake PVG model -------------------------------------------------------------------------------------------------------------------
class FakePVGModel(torch.nn.Module):
    """The getters `HipPeriodicVibrationGaussianRenderer` (and the reference's renderer) call, over parameters that store activated
    values; `config` carries cycle, velocity_decay and time_duration."""

    def __init__(self, means, scales, quats, opacities, shs, velocity, t, scale_t, cycle=0.2, velocity_decay=1.0, active_sh_degree=3):
        super().__init__()
        P = torch.nn.Parameter
        self.means, self.scales_, self.rotations_, self.opacities_, self.shs = P(means), P(scales), P(quats), P(opacities), P(shs)
        self.velocity, self.t, self.scale_t_ = P(velocity), P(t), P(scale_t)
        self.config = types.SimpleNamespace(cycle=cycle, velocity_decay=velocity_decay, time_duration=(-0.5, 0.5))
        self.active_sh_degree = active_sh_degree
        self.max_sh_degree = int(math.isqrt(shs.shape[1])) - 1
        self.is_pre_activated = False

    get_xyz = property(lambda s: s.means)
    get_scaling = property(lambda s: s.scales_)
    get_rotation = property(lambda s: s.rotations_)
    get_opacity = property(lambda s: s.opacities_)
    get_features = property(lambda s: s.shs)

    def get_means(self): return self.means
    def get_scales(self): return self.scales_
    def get_rotations(self): return self.rotations_
    def get_opacities(self): return self.opacities_
    def get_velocity(self): return self.velocity
    def get_t(self): return self.t
    def get_scale_t(self): return self.scale_t_

    def get_mean_SHM(self, t):
        a = 1 / self.config.cycle * torch.pi * 2
        return self.get_means() + self.get_velocity() * torch.sin((t - self.get_t()) * a) / a

    def get_marginal_t(self, timestamp):
        return torch.exp(-0.5 * (self.get_t() - timestamp) ** 2 / self.get_scale_t() ** 2)

    def get_average_velocity(self):
        return self.get_velocity() * torch.exp(-self.get_scale_t() / self.config.cycle / 2 * self.config.velocity_decay)

    def leaves(self):
        return {"means": self.means, "velocity": self.velocity, "t": self.t, "scale_t": self.scale_t_, "opacities": self.opacities_}


def pvg_scene(n=200, seed=5, scale=15.0):
    """A small dynamic scene (float32, CPU): the synthetic splats of the other renderer tests plus seeded PVG rows whose lifespans keep
    most splats visible at time 0.5 + time_offset."""
    from oracle import gsplat_oracle as O
    means, scales, quats, opac, shs = O.synthetic_scene(n, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    velocity = torch.randn(n, 3, generator=g) * 0.5
    t = (torch.rand(n, 1, generator=g) * 1.2 - 0.1) - 0.5
    scale_t = torch.exp(-3.0 * torch.rand(n, 1, generator=g))
    return dict(means=means, scales=scales * scale, quats=quats, opacities=opac, shs=shs, velocity=velocity, t=t, scale_t=scale_t)

"""EvaluateBSDF against an independent float64 restatement (the furnace value of the default dielectric
was only "pinned" by a measured band).

The oracle's Material code (oracle.cpp eval_bsdf and the lobes it mixes) is held against a numpy float64 version written from
the reference text alone — Material.slang:167-254 (EvaluateBSDF), 256-308 (diffuse / metallic / dielectric reflection),
331-387 (EvaluateReflection / EvaluateRefraction), 394-423 (GGX D, Lambda, G1), 425-449 (Schlick / dielectric Fresnel), 39-77
(Initialize: Ax, Ay, Eta) — with its own lookup-table sampler (LINEAR / CLAMP_TO_EDGE, layer = round-half-even; numpy indexing,
not the contract's texel_coords) on the tables the reference ships.  It also settles what the furnace band was hiding: the
directional albedo of the default dielectric IS 1 on both sides; the energy the furnace loses is lost by the estimator."""
import numpy as np
import pytest

from test_oracle_bsdf import mat, sphere_grid


def lut64(table, u, v, layer):
    """uLookupTableSampler on an R32F 2D array (PathTracer.cpp:93-94): bilinear, clamp to edge, nearest layer (ties to even).
    A NaN coordinate (sqrt(V.z) of a view direction that a strong normal map has put below the shading plane) is left to the
    implementation by Vulkan; the project pins it as texel-space 0 (include/vpt_fp32.h texel_coords, lut_layer)."""
    sz, sy, sx = table.shape
    l = 0 if np.isnan(layer) else int(np.rint(np.clip(layer, 0, sz - 1)))
    def axis(c, n):
        x = np.asarray(c, np.float64) * n - 0.5
        x = np.where(np.abs(x) < 1e9, x, 0.0)
        f = np.floor(x)
        return np.clip(f, 0, n - 1).astype(int), np.clip(f + 1, 0, n - 1).astype(int), x - f
    x0, x1, fx = axis(u, sx); y0, y1, fy = axis(v, sy)
    t = table[l].astype(np.float64)
    a = t[y0, x0] + (t[y0, x1] - t[y0, x0]) * fx
    b = t[y1, x0] + (t[y1, x1] - t[y1, x0]) * fx
    return a + (b - a) * fy


class Mat64:
    def __init__(self, d, luts, inside=False, ec=True):
        self.base = np.array(d["base_color"], np.float64); self.spec = np.array(d["specular_color"], np.float64)
        self.metallic, self.rough, self.trans, self.aniso = float(d["metallic"]), float(d["roughness"]), float(d["transmission"]), float(d["anisotropy"])
        self.ior = max(float(np.float32(d["ior"])), 1.000001)
        aspect = np.sqrt(1.0 - np.sqrt(self.aniso) * 0.9)
        self.ax, self.ay = max(1e-5, self.rough / aspect), max(1e-5, self.rough * aspect)
        self.eta = self.ior if inside else 1.0 / self.ior
        self.luts, self.ec = luts, ec

    def D(self, H):
        return 1.0 / (np.pi * self.ax * self.ay * (H[:, 0] ** 2 / self.ax ** 2 + H[:, 1] ** 2 / self.ay ** 2 + H[:, 2] ** 2) ** 2)

    def G1(self, W):
        lam = (-1.0 + np.sqrt(1.0 + (self.ax ** 2 * W[:, 0] ** 2 + self.ay ** 2 * W[:, 1] ** 2) / np.abs(W[:, 2]) ** 2)) / 2.0
        return 1.0 / (1.0 + lam)

    def fresnel(self, c):
        st2 = self.eta ** 2 * (1.0 - c * c)
        ct = np.sqrt(np.maximum(1.0 - st2, 0.0))
        rs = (self.eta * ct - c) / (self.eta * ct + c); rp = (self.eta * c - ct) / (self.eta * c + ct)
        return np.where(st2 > 1.0, 1.0, 0.5 * (rs * rs + rp * rp))

    def reflection(self, V, L, F):
        Vn = np.broadcast_to(V, L.shape)
        H = Vn + L; H = H / np.linalg.norm(H, axis=1, keepdims=True)
        VdotH = (Vn * H).sum(1)
        D, GV, GL = self.D(H), self.G1(Vn), self.G1(L)
        ok = L[:, 2] > 1e-5
        pdf = np.where(ok, (GV * np.maximum(VdotH, 0.0) * D / V[2]) / (4.0 * VdotH), 0.0)
        f = np.where(ok[:, None], (D * GV * GL / (4.0 * V[2]))[:, None] * F, 0.0)
        return f, pdf

    def evaluate(self, V, L):
        V = np.asarray(V, np.float64); L = np.asarray(L, np.float64)
        Vn = np.broadcast_to(V, L.shape)
        pm, pd, pg = self.metallic, (1 - self.metallic) * (1 - self.trans), (1 - self.metallic) * self.trans
        s = pm + pd + pg; pm, pd, pg = pm / s, pd / s, pg / s
        refr = L[:, 2] < 0.0
        Hr = self.eta * Vn + L; Hr = Hr / np.linalg.norm(Hr, axis=1, keepdims=True); Hr = np.where(Hr[:, 2:3] < 0, -Hr, Hr)
        Hh = Vn + L; Hh = Hh / np.linalg.norm(Hh, axis=1, keepdims=True)
        H = np.where(refr[:, None], Hr, Hh)
        VdotH, LdotH = (Vn * H).sum(1), (L * H).sum(1)
        valid_refr = refr & (((VdotH > 0) & (LdotH < 0)) | ((VdotH < 0) & (LdotH > 0)))
        F = self.fresnel(np.abs(VdotH))
        f = np.zeros_like(L); pdf = np.zeros(len(L))
        if self.ec:
            gec = float(lut64(self.luts[2] if self.eta > 1.0 else self.luts[1], np.sqrt(V[2]), self.rough, (np.clip(self.ior, 1.0001, 2.0) - 1.0) * 32.0))
            e_r = float(lut64(self.luts[0], V[2], self.rough, self.aniso * 32.0))
        up = ~refr
        # metallic: F = lerp(base, specular, Schlick(V.H)), energy compensation (1 + base * (1 - E) / E)
        m5 = np.clip(1.0 - (Vn * Hh).sum(1), 0.0, 1.0) ** 5
        Fm = self.base[None, :] + (self.spec - self.base)[None, :] * m5[:, None]
        fm, pm_ = self.reflection(V, L, Fm)
        if self.ec:
            fm = (1.0 + self.base * ((1.0 - e_r) / e_r))[None, :] * fm
        f += np.where(up[:, None], fm * pm, 0.0); pdf += np.where(up, pm_ * pm, 0.0)
        # diffuse
        fd = (self.base / np.pi)[None, :] * L[:, 2:3]; pdd = L[:, 2] / np.pi * (L[:, 2] > 0)
        f += np.where(up[:, None], fd * (pd * (1 - F))[:, None], 0.0); pdf += np.where(up, pdd * pd * (1 - F), 0.0)
        # dielectric specular
        fs, ps = self.reflection(V, L, self.spec[None, :])
        if self.ec:
            fs = fs / e_r
        f += np.where(up[:, None], fs * (pd * F)[:, None], 0.0); pdf += np.where(up, ps * pd * F, 0.0)
        # glass reflection
        fg, pgl = self.reflection(V, L, self.spec[None, :])
        if self.ec and gec > 0.01:
            fg = fg / gec
        f += np.where(up[:, None], fg * (pg * F)[:, None], 0.0); pdf += np.where(up, pgl * pg * F, 0.0)
        # glass refraction
        den2 = (LdotH + self.eta * VdotH) ** 2
        eta2 = self.eta ** 2
        D, GV, GL = self.D(H), self.G1(Vn), self.G1(L)
        okr = valid_refr & (L[:, 2] < 1e-5)
        with np.errstate(all="ignore"):
            pr = (GV * np.abs(VdotH) * D / V[2]) * (eta2 * np.abs(LdotH) / den2)
            fr = (D * GV * GL * eta2 / den2 * (np.abs(VdotH) * np.abs(LdotH) / abs(V[2])))[:, None] * self.base[None, :]
        if self.ec and gec > 0.01:
            fr = fr / gec
        f += np.where(okr[:, None], fr * (pg * (1 - F))[:, None], 0.0); pdf += np.where(okr, pr * pg * (1 - F), 0.0)
        return f, pdf


CASES = [dict(), dict(roughness=0.4), dict(metallic=1.0, roughness=0.35, base_color=(0.9, 0.6, 0.3)), dict(metallic=0.4, roughness=0.6, anisotropy=0.5, base_color=(0.7, 0.8, 0.9)),
         dict(transmission=1.0, roughness=0.3, ior=1.5), dict(transmission=0.6, metallic=0.2, roughness=0.5, ior=1.33, base_color=(0.8, 0.9, 1.0))]


@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("cos_v", [0.95, 0.5, 0.15])
@pytest.mark.parametrize("inside", [False, True])
def test_evaluate_bsdf_equals_the_float64_restatement(vpt, oracle, kw, cos_v, inside):
    if inside and kw.get("transmission", 0.0) == 0.0:
        pytest.skip("only glass is ever evaluated from inside")
    luts = vpt.scenes.load_luts()
    d = vpt.scenes.material(**kw)
    V = np.array([np.sqrt(1 - cos_v * cos_v) * 0.8, np.sqrt(1 - cos_v * cos_v) * 0.6, cos_v], np.float32)
    rng = np.random.default_rng(11)
    L = rng.normal(size=(40000, 3)); L /= np.linalg.norm(L, axis=1, keepdims=True)
    L = L[np.abs(L[:, 2]) > 0.02].astype(np.float32)
    f32, p32 = oracle.bsdf_eval_ec(mat(vpt, **kw), V, L, luts, inside=inside)
    f64, p64 = Mat64(d, luts, inside=inside).evaluate(V.astype(np.float64), L.astype(np.float64))
    # conditioning: where the half vector of a refraction is nearly undefined (eta V + L ~ 0) or V.H ~ 0, fp32 cancellation dominates
    Ld = L.astype(np.float64); Vd = V.astype(np.float64)
    eta = (max(d["ior"], 1.000001) if inside else 1.0 / max(d["ior"], 1.000001))
    hr = np.linalg.norm(eta * Vd + Ld, axis=1); hh = np.linalg.norm(Vd + Ld, axis=1)
    ok = np.where(Ld[:, 2] < 0, hr > 0.05, hh > 0.05)
    scale = np.maximum(np.abs(f64).max(1), 1e-3)
    assert np.abs(f32 - f64).max(1)[ok].max() / 1.0 < 1e-3 * max(1.0, float(scale[ok].max()))
    rel = (np.abs(f32 - f64).max(1) / scale)[ok]
    # tolerance: fp32 evaluation of ~40 dependent operations (divisions by (L.H + eta V.H)^2 in the refraction lobe): 5e-4 relative for
    # 99.9 % of the directions, 5e-3 for the worst one
    assert np.quantile(rel, 0.999) < 5e-4 and rel.max() < 5e-3, (float(np.quantile(rel, 0.999)), float(rel.max()))
    relp = (np.abs(p32 - p64) / np.maximum(np.abs(p64), 1e-3))[ok]
    assert np.quantile(relp, 0.999) < 5e-4 and relp.max() < 5e-3, (float(np.quantile(relp, 0.999)), float(relp.max()))
    # the two sides agree on which directions carry anything at all, up to the sign of V.H / L.H where it is within rounding of 0
    assert ((p32 > 0)[ok] != (p64 > 0)[ok]).mean() < 1e-3


def test_directional_albedo_of_the_default_dielectric(vpt, oracle):
    """Integral of f over the hemisphere (f carries the cosine) for the default material (roughness 1, IOR 1.5, white) with energy
    compensation: 1 at every view angle, by the float64 restatement as by the oracle — diffuse * (1 - F) + specular * F / E is
    energy conserving as a BSDF.  So the 0.83 the furnace test (tests/test_oracle_kat.py) sees inside the box is NOT a property of
    EvaluateBSDF: it comes from the estimator, whose pdf is not the density SampleBSDF draws from (lobe chosen with F(V.H_sampled),
    evaluated with F(V.H_(V+L)), below-horizon draws rejected: Material.slang:107 vs 202, 150-160; tests/test_oracle_bsdf.py)."""
    luts = vpt.scenes.load_luts()
    d = vpt.scenes.material()
    dirs, w = sphere_grid(600, 720, hemisphere=True)
    for cos_v in (0.95, 0.6, 0.25):
        V = np.array([np.sqrt(1 - cos_v * cos_v), 0.0, cos_v], np.float32)
        f32, _ = oracle.bsdf_eval_ec(mat(vpt), V, dirs, luts)
        f64, _ = Mat64(d, luts).evaluate(V.astype(np.float64), dirs.astype(np.float64))
        a32, a64 = float(f32[:, 0].astype(np.float64).sum() * w), float(f64[:, 0].sum() * w)
        assert abs(a32 - a64) < 2e-4, (cos_v, a32, a64)
        assert abs(a64 - 1.0) < 3e-3, (cos_v, a64)   # the shipped reflection table is E[f / pdf] of the specular lobe, to its Monte-Carlo error
        # ... while the estimator the integrator runs, f / pdf over SampleBSDF's draws, returns 4-6 % less per bounce: 2.5-6 % of the
        # draws are rejected (pdf 0) and the rest carry f / pdf ~ 1.  0.96 per bounce over the 4-5 bounces of a path in the box = 0.83.
        Ls, fs, ps = oracle.bsdf_sample_ec(mat(vpt), V, 5, 200000, luts)
        okd = ps > 0
        est = float((fs[okd, 0] / ps[okd]).sum() / len(ps))
        assert 0.94 < est < 0.985 and est < a64 - 0.015 and 0.93 < okd.mean() < 0.98, (cos_v, est, float(okd.mean()))


# ---------------------------------------------------------------- the sampler, restated: same PCG stream, float64 geometry
def _pcg(s):
    s = np.uint64(s)
    state = (s * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xffffffff)
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & np.uint64(0xffffffff)
    return int((word >> np.uint64(22)) ^ word)


class Rng64:
    def __init__(self, seed): self.s = int(seed) & 0xffffffff
    def raw(self):   # Sampler.PCG(): the next hash itself (what the jittered density-grid lookups take modulo 3)
        self.s = _pcg(self.s)
        return self.s
    def uf(self):   # Sampler.slang:38-43: float(hash) / float(UINT_MAX); float(UINT_MAX) is 2^32 in fp32
        self.s = _pcg(self.s)
        return float(np.float32(self.s)) / 4294967296.0


def _norm(v): return v / np.sqrt((v * v).sum())


def sample64(m, V, rng):
    """GGXSampleAnisotopic (Sampler.slang:141-166) + SampleBSDF (Material.slang:94-165) + EvaluateBSDF at the drawn direction."""
    u1, u2 = rng.uf(), rng.uf()
    Vh = _norm(np.array([m.ax * V[0], m.ay * V[1], abs(V[2])]))
    lensq = Vh[0] ** 2 + Vh[1] ** 2
    T1 = np.array([-Vh[1], Vh[0], 0.0]) / np.sqrt(lensq) if lensq > 0 else np.array([1.0, 0.0, 0.0])
    T2 = np.cross(Vh, T1)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    t1, t2 = r * np.cos(phi), r * np.sin(phi)
    s = 0.5 * (1.0 + Vh[2])
    t2 = (1.0 - s) * np.sqrt(1.0 - t1 * t1) + s * t2
    Nh = t1 * T1 + t2 * T2 + np.sqrt(max(0.0, 1.0 - t1 * t1 - t2 * t2)) * Vh
    H = _norm(np.array([m.ax * Nh[0], m.ay * Nh[1], max(0.0, Nh[2])]))
    pm, pd, pg = m.metallic, (1 - m.metallic) * (1 - m.trans), (1 - m.metallic) * m.trans
    tot = pm + pd + pg; pm, pd, pg = pm / tot, pd / tot, pg / tot
    F = float(m.fresnel(np.array([float(np.dot(V, H))]))[0])
    x1 = rng.uf()
    refl = lambda: _norm(-V - 2.0 * np.dot(H, -V) * H)
    refracted = False
    if x1 < pm:
        L = refl()
    elif x1 < pm + pd:
        if rng.uf() < F:
            L = refl()
        else:   # RandomHemisphereVecCosineWeight: normalize(RandomSphereVec() + n)
            a1, a2 = rng.uf(), rng.uf()
            th = 2.0 * np.pi * a1; z = 1.0 - 2.0 * a2; rr = np.sqrt(1.0 - z * z)
            L = _norm(np.array([rr * np.cos(th), rr * np.sin(th), z]) + np.array([0.0, 0.0, 1.0]))
    else:
        if rng.uf() < F:
            L = refl()
        else:
            I = -V; ni = float(np.dot(H, I)); k = 1.0 - m.eta ** 2 * (1.0 - ni * ni)
            L = _norm(I * m.eta - H * (m.eta * ni + np.sqrt(k))) if k >= 0 else np.zeros(3)
            refracted = True
    if (L[2] < 0.0 and not refracted) or (refracted and L[2] >= 0.0):
        return None
    return L


@pytest.mark.parametrize("kw", [dict(), dict(metallic=1.0, roughness=0.35), dict(roughness=0.3, anisotropy=0.6), dict(transmission=1.0, roughness=0.3, ior=1.5),
                                dict(transmission=0.5, metallic=0.3, roughness=0.5, ior=1.4)])
def test_sampler_draws_equal_the_float64_restatement(vpt, oracle, kw):
    """VNDF sampling + SampleBSDF: the oracle's draws (one PCG stream, variable number of draws per sample) against a float64
    restatement fed by an independent implementation of the same hash chain: same lobe decisions, same rejections, directions
    within 2e-5 — except where a decision hangs on a comparison within float32 rounding of a draw (counted, < 0.2 %)."""
    luts = vpt.scenes.load_luts()
    d = vpt.scenes.material(**kw)
    m = Mat64(d, luts, ec=False)
    V = np.array([0.48, 0.36, 0.8], np.float32)
    n = 4000
    L32, f32, p32 = oracle.bsdf_sample(mat(vpt, **kw), V, 77, n)
    rng = Rng64(77)
    V64 = V.astype(np.float64)
    bad = 0
    for i in range(n):
        L = sample64(m, V64, rng)
        ok32 = p32[i] > 0
        if L is None:
            same = not ok32 or f32[i].max() == 0
        else:
            same = bool(np.abs(L - L32[i]).max() < 2e-5)
            if same and ok32:   # the sample's value is EvaluateBSDF there
                f64, p64 = m.evaluate(V64, L[None, :])
                same = abs(p64[0] - p32[i]) <= 2e-4 * max(1.0, abs(p64[0])) + 1e-6
        if not same:
            bad += 1   # (a flipped decision would also shift the stream: every later draw would differ and the bound below would fail)
    assert bad <= 0.002 * n, bad

"""Every shape of the fused bloom/tonemap schedule against the oracle.

enqueue_post (csrc/api_post.hip) assembles the fused schedule per call from the image's mip sizes and mip_count; which kernels run,
with how many levels each, is restated by tests/post_plan.py.  CASES is chosen with that restatement so that every launch kind and
level count the schedule can produce is run here — tests/test_post_plan_cpu.py fails, naming the element, if the table stops
covering what a sweep of sizes reaches — and each case proves on the device, through the launch counters, that it ran the launches
the restatement says it runs.  Everything is compared for equality: RGBA8 byte for byte, bloom mip 0 bit for bit."""
import numpy as np
import pytest

import post_plan

pytestmark = pytest.mark.gpu

# (width, height, mip_count): the plan of each is in the comment (post_plan.plan)
CASES = [
    (3401, 541, 8),     # first, down_chain 3, tail staged 3, up_chain 4, final up
    (3401, 18, 4),      # first, down, tail staged 1, up_chain 2, final up
    (255, 541, 6),      # first, down_chain 2, tail staged 2, up_chain 3, final up
    (64, 68, 6),        # first, tail staged 4, up, final up
    (2047, 18, 4),      # first, tail plain 2, final up
    (4, 4, 1),          # final noup
    (4, 5, 2),          # first, final up
    (131, 135, 7),      # first, tail staged 5, up, final up
    (3401, 10, 3),      # first, tail plain 1, final up
    (2047, 68, 6),      # first, down, tail plain 3, up, final up
    (1023, 1023, 10),   # every level odd in both dimensions: first, down_chain 3, tail staged 4, up_chain 4, final up
    (511, 511, 10),     # every level odd in both dimensions: first, down_chain 2, tail staged 4, up_chain 3, final up
    (16, 2160, 4),      # one block column in the up chain: first, down, tail staged 1, up_chain 2, final up
    (2160, 16, 4),      # one block row in the up chain (same plan)
    (64, 2160, 4),      # no tail, one block column in the down chain: first, down_chain 2, up_chain 2, final up
    (135, 255, 3),      # no tail, single launches only: first, down, up, final up
    (18, 1920, 4),      # plain tail whose base is even in both dimensions: first, tail plain 2, final up
]
# a second parameter set, far from the defaults in every field the post chain reads
CUSTOM = dict(bloom_strength=0.7, bloom_threshold=0.6, falloff_range=0.35, exposure=1.7, gamma=1.9)


def hdr_image(w, h, seed):
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w, 4), np.float32)
    img[..., :3] = rng.gamma(0.4, 4.0, (h, w, 3))
    img[rng.rand(h, w) < 0.01, :3] *= 200.0  # fireflies above the bloom threshold
    img[..., 3] = 1.0
    return img


def tap_flags(vpt, linear):
    f = vpt._abi.FLAGS_DEFAULT
    return f if linear else f & ~vpt._abi.FLAG_TONEMAP_LINEAR_BLOOM_TAP


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_counted(g, pp, want_bloom):
    """One vpt_postprocess and the bloom / tonemap launches it made."""
    g.reset_stats()
    r = g.postprocess(pp, want_bloom=want_bloom)
    kl = g.stats()["kernel_launches"]
    return r, (kl["bloom"], kl["tonemap"])


@pytest.mark.parametrize("w,h,mips", CASES, ids=["%dx%d-m%d" % c for c in CASES])
def test_case_matches_oracle_and_plan(vpt, oracle, w, h, mips):
    img = hdr_image(w, h, 3 * w + h)
    fused_launches = post_plan.predicted_launches(w, h, mips)
    ref_launches = post_plan.reference_launches(w, h, mips)
    assert ref_launches == (1 + 2 * (min(mips, len(post_plan.mip_sizes(w, h))) - 1), 1)
    g = vpt.PathTracer(w, h)
    try:
        for linear in (True, False):
            flags = tap_flags(vpt, linear)
            g.set_params(vpt.default_params(flags=flags))
            g.set_radiance(img, 1)
            for kw in ({}, CUSTOM):
                what = "%dx%d mips %d %s tap %r" % (w, h, mips, "linear" if linear else "nearest", kw)
                ref8, refb = oracle.postprocess(img, vpt.default_post_params(mip_count=mips, **kw), flags)
                for schedule, launches in ((0, fused_launches), (1, ref_launches)):
                    pp = vpt.default_post_params(mip_count=mips, schedule=schedule, **kw)
                    (out8, bloom), n_bloom = run_counted(g, pp, True)
                    only8, n_plain = run_counted(g, pp, False)   # the fused schedule skips the mip-0 store when nobody asks for it
                    assert n_bloom == launches and n_plain == launches, (what, schedule, n_bloom, n_plain, launches, post_plan.plan(w, h, mips))
                    assert np.array_equal(bits(bloom), bits(refb)), (what, schedule, "bloom mip 0")
                    assert np.array_equal(out8, ref8), (what, schedule, "rgba8 (bloom wanted)")
                    assert np.array_equal(only8, ref8), (what, schedule, "rgba8 (bloom not wanted)")
    finally:
        g.close()


def test_one_context_many_calls(vpt, oracle):
    """A host calls the post chain again and again on one context: other schedule, other mip_count, other parameters, a new image, a
    new size.  Nothing of an earlier call — mip levels a shorter chain does not rewrite, the previous RGBA8 image, buffers of the
    previous size — may show in a later one."""
    A, B = (301, 173), (2047, 68)          # A: staged tails; B: plain tails (mips 10 -> `tail plain 3`, 4 -> `tail plain 1`, 3 -> no tail)
    assert any(e.startswith("tail staged") for e in post_plan.plan(*A, 10)) and any(e.startswith("tail plain") for e in post_plan.plan(*B, 10))
    assert any(e.startswith("tail plain") for e in post_plan.plan(*B, 4)) and not any(e.startswith("tail") for e in post_plan.plan(*B, 3))
    imgs = {"a1": hdr_image(*A, 11), "a2": hdr_image(*A, 12), "b1": hdr_image(*B, 13), "b2": hdr_image(*B, 14)}
    steps = [  # ("image", name) | ("resize", size) | ("post", schedule, mip_count, want_bloom, other parameters)
        ("image", "a1"),
        ("post", 0, 10, True, {}), ("post", 1, 3, True, {}), ("post", 0, 7, False, {}), ("post", 0, 1, True, {}), ("post", 1, 10, False, {}),
        ("post", 0, 3, True, CUSTOM), ("post", 0, 10, False, CUSTOM), ("post", 1, 7, True, {}), ("post", 0, 1, False, {}), ("post", 0, 10, True, {}),
        ("image", "a2"),
        ("post", 0, 10, False, {}), ("post", 0, 10, True, {}), ("post", 1, 1, True, {}), ("post", 0, 4, True, dict(bloom_strength=0.5)),
        ("resize", B), ("image", "b1"),
        ("post", 0, 10, True, {}), ("post", 0, 3, False, {}), ("post", 1, 10, True, {}), ("post", 0, 4, True, CUSTOM), ("post", 0, 1, True, {}), ("post", 0, 10, False, {}),
        ("image", "b2"),
        ("post", 0, 4, False, {}), ("post", 0, 10, True, {}),
        ("resize", A), ("image", "a1"),
        ("post", 0, 10, True, {}), ("post", 0, 3, False, {}), ("post", 1, 10, True, {}), ("post", 0, 7, True, CUSTOM),
    ]
    cache = {}

    def expect(name, mips, kw):
        key = (name, mips, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = oracle.postprocess(imgs[name], vpt.default_post_params(mip_count=mips, **kw))
        return cache[key]

    g = vpt.PathTracer(*A)
    try:
        size, name = A, None
        for n, step in enumerate(steps):
            if step[0] == "image":
                name = step[1]
                g.set_radiance(imgs[name], 1)
            elif step[0] == "resize":
                size = step[1]
                g.resize(*size)
            else:
                _, schedule, mips, want_bloom, kw = step
                pp = vpt.default_post_params(schedule=schedule, mip_count=mips, **kw)
                ref8, refb = expect(name, mips, kw)
                launches = post_plan.predicted_launches(*size, mips) if schedule == 0 else post_plan.reference_launches(*size, mips)
                r, counted = run_counted(g, pp, want_bloom)
                out8, bloom = r if want_bloom else (r, None)
                assert counted == launches, (n, step, counted, launches)
                assert np.array_equal(out8, ref8), (n, step, "rgba8")
                if want_bloom:
                    assert np.array_equal(bits(bloom), bits(refb)), (n, step, "bloom mip 0")
        # the asynchronous form leaves the same image on the device
        pp = vpt.default_post_params(mip_count=7, **CUSTOM)
        blocking = g.postprocess(pp)
        g.postprocess(vpt.default_post_params(mip_count=1))          # something else in the output image in between
        ticket = g.postprocess_device(pp)
        g.wait(ticket)
        assert np.array_equal(g.output_to_host(), blocking) and np.array_equal(blocking, expect("a1", 7, CUSTOM)[0])
    finally:
        g.close()


# ---- non-finite and negative input

def special_image(w, h, seed):
    """An HDR image with isolated special texels: the four corners and seven places inside."""
    img = hdr_image(w, h, seed)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    big, den = np.float32(3e38), np.float32(1e-40)
    assert den != 0 and den < np.finfo(np.float32).tiny
    at = lambda fx, fy: (min(h - 1, int(fy * h)), min(w - 1, int(fx * w)))
    img[0, 0, :3] = inf
    img[0, w - 1, :3] = nan
    img[h - 1, 0, :3] = -inf
    img[h - 1, w - 1, :3] = big                            # finite, but any sum of two of them is not
    img[at(0.13, 0.35)][:3] = (-5.0, -0.25, -40.0)
    img[at(0.23, 0.65)][:3] = (-0.0, -0.0, -0.0)
    img[at(0.34, 0.45)][:3] = (den, -den, den)
    img[at(0.47, 0.25)][:3] = (1.0, nan, 2.0)              # one channel only
    img[at(0.61, 0.75)][:3] = (0.5, 0.25, inf)
    img[at(0.74, 0.55)][:3] = (-big, 1.0, big)
    img[at(0.87, 0.35)][:3] = (big, big, -0.0)
    return img


# (width, height, mip_count): the deeper the chain, the further one non-finite texel spreads through the blurs, so the chains are short
SPECIAL_CASES = [
    (3401, 10, 3),    # first, tail plain 1, final up
    (2047, 18, 4),    # first, tail plain 2, final up
    (2047, 68, 4),    # first, down, tail plain 1, up, final up
    (301, 173, 4),    # first, down, tail staged 1, up, final up
    (301, 173, 2),    # first, final up
    (301, 173, 1),    # final noup
]
SPECIAL_PARAMS = [{}, dict(falloff_range=0.0), dict(bloom_strength=0.0), dict(exposure=0.0), dict(CUSTOM)]
MAX_NONFINITE = 0.25   # of the oracle's bloom mip 0: beyond that the comparison would mostly be NaN against NaN


@pytest.mark.parametrize("w,h,mips", SPECIAL_CASES, ids=["%dx%d-m%d" % c for c in SPECIAL_CASES])
def test_nonfinite_and_negative_input(vpt, oracle, w, h, mips):
    """inf, NaN, negative, -0.0, denormal and near-overflow texels, and the parameter values that make 0/0 (falloff_range = 0 in the soft
    threshold), 0 * inf (bloom_strength = 0) and 0 * x (exposure = 0).  include/vpt_fp32.h pins unorm8(NaN), pow_ and min/max on NaN, so
    RGBA8 is byte-exact in both schedules; bloom mip 0 has its NaNs where the oracle has them (payloads are not compared) and equals it
    bit for bit everywhere else."""
    plan = post_plan.plan(w, h, mips)
    img = special_image(w, h, w + mips)
    g = vpt.PathTracer(w, h)
    try:
        for linear in (True, False):
            flags = tap_flags(vpt, linear)
            g.set_params(vpt.default_params(flags=flags))
            g.set_radiance(img, 1)
            for kw in SPECIAL_PARAMS:
                what = "%dx%d mips %d %s tap %r" % (w, h, mips, "linear" if linear else "nearest", kw)
                ref8, refb = oracle.postprocess(img, vpt.default_post_params(mip_count=mips, **kw), flags)
                bad = ~np.isfinite(refb[..., :3]).all(axis=-1)
                print("%s: %.2f %% of the oracle's bloom mip 0 is not finite" % (what, 100.0 * bad.mean()))
                assert bad.mean() <= MAX_NONFINITE, what
                refnan = np.isnan(refb)
                for schedule in (0, 1):
                    pp = vpt.default_post_params(mip_count=mips, schedule=schedule, **kw)
                    (out8, bloom), counted = run_counted(g, pp, True)
                    only8 = g.postprocess(pp)
                    assert counted == (post_plan.predicted_launches(w, h, mips) if schedule == 0 else post_plan.reference_launches(w, h, mips)), (what, plan)
                    assert np.array_equal(np.isnan(bloom), refnan), (what, schedule, "NaN positions of bloom mip 0")
                    assert np.array_equal(bits(bloom)[~refnan], bits(refb)[~refnan]), (what, schedule, "bloom mip 0")
                    assert np.array_equal(out8, ref8), (what, schedule, "rgba8 (bloom wanted)")
                    assert np.array_equal(only8, ref8), (what, schedule, "rgba8 (bloom not wanted)")
    finally:
        g.close()


@pytest.mark.parametrize("w,h", [(64, 68), (2047, 68)])
def test_mip_count_is_clamped(vpt, oracle, w, h):
    """mip_count 0 is 1; a mip_count beyond the chain the image allows is the chain's full length."""
    full = len(post_plan.mip_sizes(w, h))
    img = hdr_image(w, h, 5)
    g = vpt.PathTracer(w, h)
    try:
        g.set_radiance(img, 1)
        for asked, means in ((0, 1), (4000, full), (full + 1, full)):
            ref8, refb = oracle.postprocess(img, vpt.default_post_params(mip_count=means))
            for schedule in (0, 1):
                (out8, bloom), counted = run_counted(g, vpt.default_post_params(mip_count=asked, schedule=schedule), True)
                assert counted == (post_plan.predicted_launches(w, h, means) if schedule == 0 else post_plan.reference_launches(w, h, means)), (asked, schedule)
                assert np.array_equal(out8, ref8) and np.array_equal(bits(bloom), bits(refb)), (asked, schedule)
    finally:
        g.close()

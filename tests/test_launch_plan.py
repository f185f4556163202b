"""csrc/msk_plan.h on a CPU: the launch plan, the regions' shares of a pass and the parts of the pool, as printed by
tests/native/launch_plan_check.cpp, against a transcription of the code the plan replaced.

THE REFERENCE is the transcription below, written from csrc/msk_gpu.hip at commit 57e7c43 and never from msk_plan.h:
  launch_trace, lines 831-868      which traversal kernel, its LDS bytes, its grid
  run_wavefront, lines 910-954     trace_split, cull, diffuse_only, sort_on, the shading LDS, the fused kernels' flags and offsets
  run_wavefront, lines 1028-1056   the fused and the shading ladders (which instantiation)
  run_wavefront, line 1216         the lane_refill of msk_stats::bytes_trace
  run_wavefront, lines 886-892     a region's share of a pass (and 1137-1147, the same sum for a part)
  run_wavefront, lines 1156-1160   the parts of the pool
Every field of every case is compared (the two lines are compared as text)."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("in_mode lds_scene in_lds_tables all_diffuse has_regular has_dielectric cull_ok in_trace_lds in_shade_lds region_size aov_groups aov_rgb | "
          "lds_tables diffuse_only regular dielectric shade_kernel sort_on shade_lds_bytes trace_kernel trace_mode refill max_inner queue_refill "
          "trace_lds_bytes bits_off trace_waves trace_split lane_refill fused_ok fused_h fused_all fused_kernel fused_iters fused_tail_pct "
          "fused_lds_bytes fused_queue_f4 fused_trace_f4 cull sync_group timing_every")

KNOB_SETS = [{}, {"MSK_TRACE_REFILL": "0"}, {"MSK_TRACE_REFILL": "16"}, {"MSK_TRACE_REFILL": "48"}, {"MSK_TRACE_QUEUE": "0"}, {"MSK_TRACE_QUEUE": "100"},
             {"MSK_SORT": "0"}, {"MSK_FUSED": "1"}, {"MSK_FUSED_HBM": "0"}, {"MSK_FUSED_TAIL_PCT": "50"}, {"MSK_CAMERA_CULL": "0"},
             {"MSK_FORCE_GENERAL_SHADE": "1"}, {"MSK_TRACE_SPLIT": "4"}]
# {shade_lds_bytes, trace_lds_bytes}.  With 1024 slots per region each 64 KB limit is met exactly and missed by one float4:
#   sort     shade_lds + 4 * 3 * 1024 <= 65536           <=> shade_lds <= 53248
#   lds_q    trace_lds + 4 * 1024 / 8 <= 65536           <=> trace_lds <= 65024
#   fused    shade_lds + trace_lds <= 65536              <=> trace_lds <= 40960 at shade_lds = 24576
# and the other region sizes move the first two limits across the remaining values (256: everything sorts; 8192: 4096 B of bits)
LDS = [(24576, 8192), (53248, 8192), (53264, 8192), (24576, 65024), (24576, 65040), (24576, 40960), (24576, 40976)]
REGION_SIZES = [256, 1024, 2048, 8192]
MSK_BLOCK, MSK_WAVE, MSK_DONE_Q_F4 = 256, 64, 128 * 5 // 2          # msk_kernels.h


def cases():
    """The cross product, in the order launch_plan_check walks it."""
    for mode, flags, aov, rs, (shade_lds, trace_lds) in itertools.product(range(7), range(32), range(4), REGION_SIZES, LDS):
        yield dict(mode=mode, lds_scene=mode in (0, 3), lds_tables=bool(flags & 1), all_diffuse=bool(flags & 2), has_regular=bool(flags & 4),
                   has_dielectric=bool(flags & 8), cull_ok=bool(flags & 16), trace_lds=trace_lds, shade_lds=shade_lds, region_size=rs,
                   aov_groups=2 if aov & 1 else 0, aov_rgb=bool(aov & 2))


def parent_plan(env, mode, lds_scene, lds_tables, all_diffuse, has_regular, has_dielectric, cull_ok, trace_lds, shade_lds, region_size, aov_groups, aov_rgb):
    """msk_gpu.hip at 57e7c43, statement by statement; `env` is the process environment of the render."""
    def env_u32(name, default):                                   # lines 781-784
        v = env.get(name)
        return int(v) if v else default
    aov_n_groups = bool(aov_groups)                                # `aov && aov->n_groups`
    # ---- run_wavefront
    trace_split = max(1, env_u32("MSK_TRACE_SPLIT", 2)) if mode == 0 else 1                                           # 910
    cull = cull_ok and not aov_rgb and not aov_n_groups and env_u32("MSK_CAMERA_CULL", 1) != 0                        # 919
    force_general = env_u32("MSK_FORCE_GENERAL_SHADE", 0) != 0                                                        # 922
    diffuse_only = all_diffuse and not aov_rgb and not aov_n_groups and not force_general                             # 924
    sort_lds = (MSK_BLOCK // MSK_WAVE) * 3 * region_size                                                              # 926
    sort_on = (not diffuse_only and (not all_diffuse or force_general) and region_size <= 4096 and bool(env_u32("MSK_SORT", 1))
               and shade_lds + sort_lds <= 64 * 1024)                                                                 # 927-928
    shade_launch_lds = shade_lds + (sort_lds if sort_on else 0) + env_u32("MSK_SHADE_PAD_LDS_KB", 0) * 1024           # 930, 932, 1049
    group = env_u32("MSK_SYNC_GROUP", 8)                                                                              # 931
    every = max(1, env_u32("MSK_TIMING_EVERY", 1))                                                                    # 937
    fused_queue_f4 = (shade_lds - (MSK_BLOCK // MSK_WAVE) * MSK_DONE_Q_F4 * 16) // 16                                 # 942
    fused_trace_f4 = shade_lds // 16                                                                                  # 943
    fused_lds = shade_lds + trace_lds                                                                                 # 944
    fused_h = mode == 6 and not lds_tables and env_u32("MSK_FUSED_HBM", 1) != 0                                       # 950
    fused_ok = ((mode == 0 and lds_tables) or fused_h) and fused_lds <= 64 * 1024 and not aov_n_groups                # 951
    fused_all = fused_ok and env_u32("MSK_FUSED", 0) != 0                                                             # 952
    fused_iters = max(1, env_u32("MSK_FUSED_ITERS", 16))                                                              # 953
    fused_tail_pct = env_u32("MSK_FUSED_TAIL_PCT", 2 if fused_h else 10) if fused_ok else 0                           # 954
    # the fused ladder, 1032-1041
    if fused_h:
        fused = ("k_wavefront_h_d" if has_dielectric else "k_wavefront_h<true>" if diffuse_only else
                 "k_wavefront_h<false,true>" if has_regular else "k_wavefront_h<false>")
    else:
        fused = ("k_wavefront_d" if has_dielectric else "k_wavefront<true>" if diffuse_only else
                 "k_wavefront<false,true>" if has_regular else "k_wavefront<false>")
    # the shading ladder, 1050-1055
    t = int(lds_tables)
    if has_dielectric:
        shade = f"k_shade_gen_d<{t}>"
    else:
        shade = f"k_shade_gen<{t},true>" if diffuse_only else f"k_shade_gen<{t},false,true>" if has_regular else f"k_shade_gen<{t},false>"
    # ---- launch_trace
    refill_env = int(env["MSK_TRACE_REFILL"]) if "MSK_TRACE_REFILL" in env else -1                                    # 835
    max_inner = env_u32("MSK_TRACE_QUANTUM", 3)                                                                       # 836
    refill = 0 if mode == 3 else refill_env if refill_env >= 0 else (0 if mode == 0 else 16)                          # 837
    lds = trace_lds + env_u32("MSK_TRACE_PAD_LDS_KB", 0) * 1024                                                       # 838
    queue_refill = 0 if refill_env >= 0 else min(64, env_u32("MSK_TRACE_QUEUE", 32))                                  # 849
    bits_off = (lds + 15) & ~15                                                                                       # 850
    lds_q = bits_off + (MSK_BLOCK // MSK_WAVE) * (region_size // 8)                                                   # 851
    if refill > 0:                                                                                                    # 839-847
        trace, launch_lds, waves = f"k_trace_r<{mode if mode in (4, 0, 1, 5, 6) else 2}>", lds, 1
        assert mode != 3
    elif mode == 0 and queue_refill and lds_scene and lds_q <= 64 * 1024:                                             # 852-856
        trace, launch_lds, waves = "k_trace_q", lds_q, trace_split
    elif mode == 0:                                                                                                   # 857-861
        trace, launch_lds, waves = "k_trace<0>", lds, trace_split
    else:                                                                                                             # 862-867
        trace, launch_lds, waves = f"k_trace<{mode if mode in (1, 2, 4, 5, 6) else 3}>", lds, 1
    # ---- the byte count
    lane_refill = mode != 0 and mode != 3 and (int(env["MSK_TRACE_REFILL"]) != 0 if "MSK_TRACE_REFILL" in env else True)     # 1216
    b = lambda *v: " ".join(str(int(x)) if isinstance(x, bool) else str(x) for x in v)
    return (b(mode, lds_scene, lds_tables, all_diffuse, has_regular, has_dielectric, cull_ok, trace_lds, shade_lds, region_size, aov_groups, aov_rgb) + " | " +
            b(lds_tables, diffuse_only, has_regular, has_dielectric, shade, sort_on, shade_launch_lds, trace, mode, refill, max_inner, queue_refill,
              launch_lds, bits_off, waves, trace_split, lane_refill, fused_ok, fused_h, fused_all, fused, fused_iters, fused_tail_pct, fused_lds,
              fused_queue_f4, fused_trace_f4, cull, group, every))


def parent_share(total, n_regions, r):
    """lines 886-892 (and 1138-1144)"""
    n_chunks = (total + 63) // 64
    mine = (n_chunks - r + n_regions - 1) // n_regions if n_chunks > r else 0
    n = mine * 64
    if mine and (mine - 1) * n_regions + r == n_chunks - 1:
        n -= n_chunks * 64 - total
    return n


def parent_parts(n_regions, n_parts, skew_pct):
    """lines 1156-1160: [(first, last)] per part; double arithmetic, as Python's floats are"""
    skew = skew_pct / 100.0
    cum = [0.0] * (n_parts + 1)
    for k in range(n_parts):
        cum[k + 1] = cum[k] + 1.0 + skew * ((n_parts - 1) / 2.0 - k)
    return [(int(n_regions * (cum[k] / cum[n_parts])), n_regions if k + 1 == n_parts else int(n_regions * (cum[k + 1] / cum[n_parts])))
            for k in range(n_parts)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", out, os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp")])
    return out


def run(exe, what, knobs=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MSK_")}
    env.update(knobs or {})
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_plan_is_what_the_ladders_decided(exe, knobs):
    got = run(exe, "plans", knobs)
    want = [parent_plan(knobs, **c) for c in cases()]
    assert len(got) == len(want) == 7 * 32 * 4 * len(REGION_SIZES) * len(LDS)
    for g, w in zip(got, want):
        assert g == w, f"{knobs}\nfields: {FIELDS}\nplan:   {g}\nparent: {w}"


def test_the_cases_meet_every_limit_from_both_sides(exe):
    """What the cross product is for: every instantiation is chosen somewhere, and each 64 KB limit is met exactly and missed by 16 bytes."""
    f = FIELDS.split()
    default = [dict(zip(f, l.split())) for l in run(exe, "plans")]
    rows = default + [dict(zip(f, l.split())) for k in ({"MSK_TRACE_REFILL": "0"}, {"MSK_TRACE_REFILL": "16"}, {"MSK_TRACE_QUEUE": "0"}) for l in run(exe, "plans", k)]
    assert {r["trace_kernel"] for r in rows} == {"k_trace_q"} | {f"k_trace<{m}>" for m in range(7)} | {f"k_trace_r<{m}>" for m in (0, 1, 2, 4, 5, 6)}
    assert {r["shade_kernel"] for r in rows} == {k.format(t) for t in (0, 1) for k in ("k_shade_gen_d<{}>", "k_shade_gen<{},true>", "k_shade_gen<{},false,true>", "k_shade_gen<{},false>")}
    assert {r["fused_kernel"] for r in rows if r["fused_ok"] == "1"} == {k.format(h) for h in ("", "_h") for k in ("k_wavefront{}_d", "k_wavefront{}<true>", "k_wavefront{}<false,true>", "k_wavefront{}<false>")}
    pick = lambda key, **kv: {(r[key[0]], r[key[1]]) for r in default if all(r[a] == b for a, b in kv.items())}
    assert pick(("in_shade_lds", "sort_on"), region_size="1024", all_diffuse="0") >= {("53248", "1"), ("53264", "0")}
    assert pick(("in_trace_lds", "trace_kernel"), region_size="1024", in_mode="0") >= {("65024", "k_trace_q"), ("65040", "k_trace<0>")}
    assert pick(("in_trace_lds", "fused_ok"), in_mode="0", in_lds_tables="1", aov_groups="0") >= {("40960", "1"), ("40976", "0")}


def test_region_shares_add_up_and_equal_the_parents(exe):
    lines = run(exe, "shares")
    assert len(lines) == 3 * 8
    seen = set()
    for l in lines:
        v = [int(x) for x in l.split()]
        total, n, shares = v[0], v[1], v[2:]
        seen.add((total, n))
        assert len(shares) == n and sum(shares) == total
        assert sum(1 for s in shares if s % 64) <= 1
        assert shares == [parent_share(total, n, r) for r in range(n)], (total, n)
    assert seen == {(t, n) for n in (4, 1024, 6144) for t in (0, 1, 63, 64, 65, 64 * n - 1, 64 * n + 1, 2 ** 32 + 5)}


def test_parts_cover_the_pool_and_equal_the_parents(exe):
    lines = run(exe, "parts")
    seen = set()
    for l in lines:
        v = [int(x) for x in l.split()]
        n_regions, n_parts, skew, cut = v[0], v[1], v[2], v[3:]
        seen.add((n_regions, n_parts, skew))
        assert len(cut) == n_parts + 1 and cut[0] == 0 and cut[-1] == n_regions and cut == sorted(cut)      # contiguous, covering [0, n_regions)
        assert list(zip(cut[:-1], cut[1:])) == parent_parts(n_regions, n_parts, skew), (n_regions, n_parts, skew)
    assert seen == set(itertools.product((1024, 1027, 6144, 8192), (1, 2, 3, 4), (0, 10, 50)))
    # 29 / 26 / 24 / 21 % of the default pool
    cut = [int(x) for x in next(l for l in lines if l.startswith("6144 4 10 ")).split()[3:]]
    assert [round(100 * (b - a) / 6144) for a, b in zip(cut[:-1], cut[1:])] == [29, 26, 24, 21]

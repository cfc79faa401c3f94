"""Host restatement (numpy) of the device training-target sampler's draws (csrc/ngm_target.hip k_tsmv_draw / k_tsmv_rays,
include/ngm_hip.h ngm_target_sample_mv): the two field subsets and their order, the 20 sphere offsets (float32 operation by
operation, as the kernel rounds them), and the per-ray keyframe / pixel-uniform draws given each field's visible keyframes.
Test infrastructure: tests/test_gpu_target_device.py compares the device's draws with these bit for bit."""
import numpy as np

from _philox_host import philox4x32_10_words

STREAM_OBS, STREAM_RAND, STREAM_OFFSETS, STREAM_RAYS = 0x54470001, 0x54470002, 0x54470003, 0x54470004
_M = np.uint64(0xFFFFFFFF)
f32 = np.float32


def philox_words(seed, iteration, ctr, stream):
    """the four words of block `ctr` (uint64 array) of `stream` under key `seed`, offset `iteration`"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    return philox4x32_10_words(ctr & _M, ctr >> np.uint64(32), np.full_like(ctr, np.uint64(stream)),
                               np.full_like(ctr, np.uint64(int(iteration) & 0xFFFFFFFF)), int(seed) & 0xFFFFFFFF,
                               (int(seed) >> 32) & 0xFFFFFFFF)


def plan(num_current, num_fields, num_train_fields):
    n_obs = min(num_train_fields // 2, num_current)
    return n_obs, max(min(num_train_fields - n_obs, num_fields - n_obs), 0)


def draw_fields(cur, num_fields, num_train_fields, seed, iteration):
    """(subset_observed: positions in cur in draw order, subset_random: field ids in draw order, field_ids in row order)"""
    cur = np.asarray(cur, dtype=np.int64)
    n_obs, n_rand = plan(len(cur), num_fields, num_train_fields)
    key = (philox_words(seed, iteration, cur.astype(np.uint64), STREAM_OBS)[0] << np.uint64(32)) | np.arange(len(cur), dtype=np.uint64)
    sub_obs = np.argsort(key, kind="stable")[:n_obs].astype(np.int64)
    obs_ids = cur[sub_obs]
    if n_rand == 0:
        return sub_obs, np.zeros(0, np.int64), obs_ids
    f = np.arange(num_fields, dtype=np.uint64)
    key = (philox_words(seed, iteration, f, STREAM_RAND)[0] << np.uint64(32)) | f
    avail = np.ones(num_fields, bool)
    avail[obs_ids] = False
    cand = np.nonzero(avail)[0]
    sub_rand = cand[np.argsort(key[cand], kind="stable")[:n_rand]].astype(np.int64)
    return sub_obs, sub_rand, np.unique(np.concatenate([sub_rand, obs_ids]))


def log_f32(u):
    """csrc/ngm_target.hip tsmv_log, float32 operation by operation"""
    u = np.asarray(u, dtype=f32)
    b = u.view(np.uint32)
    e = (((b >> np.uint32(23)) & np.uint32(255)).astype(np.int32) - 127).astype(f32)
    m = ((b & np.uint32(0x7FFFFF)) | np.uint32(0x3F800000)).view(f32)
    s = (m - f32(1.0)) / (m + f32(1.0))
    z = s * s
    p = np.full_like(z, f32(0.0769230798))
    for c in (0.0909090936, 0.111111112, 0.142857149, 0.200000003, 0.333333343, 1.0):
        p = p * z + f32(c)
    return e * f32(0.693147182) + f32(2.0) * s * p


def sincos_2pi_f32(u):
    """csrc/ngm_target.hip tsmv_sincos_2pi: (sin 2 pi u, cos 2 pi u) for u in [0, 1), float32 operation by operation"""
    u = np.asarray(u, dtype=f32)
    u4 = u * f32(4.0)
    q = u4.astype(np.int32)
    ph = (u4 - q.astype(f32)) * f32(1.57079637)
    z = ph * ph
    ps = np.full_like(z, f32(1.60590444e-10))
    for c in (-2.50521079e-08, 2.75573188e-06, -1.98412701e-04, 8.33333377e-03, -0.166666672, 1.0):
        ps = ps * z + f32(c)
    pc = np.full_like(z, f32(2.08767570e-09))
    for c in (-2.75573188e-07, 2.48015876e-05, -1.38888892e-03, 4.16666679e-02, -0.5, 1.0):
        pc = pc * z + f32(c)
    s, c = ph * ps, pc
    sn = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    cs = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    return sn.astype(f32), cs.astype(f32)


def offsets(seed, iteration):
    """the (20, 3) normalised sphere offsets: Box-Muller on blocks 0..14 of STREAM_OFFSETS, pair p = words 2(p&1), 2(p&1)+1
    of block p >> 1, u1 = odd / 2^24"""
    p = np.arange(30)
    w = philox_words(seed, iteration, (p >> 1).astype(np.uint64), STREAM_OFFSETS)
    h = 2 * (p & 1)
    w1 = np.where(h == 0, w[0], w[2])
    w2 = np.where(h == 0, w[1], w[3])
    u1 = ((w1 >> np.uint64(9)) * np.uint64(2) + np.uint64(1)).astype(f32) * f32(1.0 / 16777216.0)
    u2 = (w2 >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0)
    r = np.sqrt(f32(-2.0) * log_f32(u1))
    sn, cs = sincos_2pi_f32(u2)
    nrm = np.stack([r * cs, r * sn], -1).reshape(20, 3)
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    n = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / n, y / n, z / n], -1).astype(f32)


def ray_draws(seed, iteration, field_ids, R, kf_mask):
    """(frame_cids (F, R) int64, u_xy (F, R, 2) float32) for the surviving fields (rows in order) given kf_mask (F, Nc)"""
    F = len(field_ids)
    fc, uxy = np.zeros((F, R), np.int64), np.zeros((F, R, 2), f32)
    for i, g in enumerate(np.asarray(field_ids, dtype=np.int64)):
        vis = np.nonzero(np.asarray(kf_mask[i]))[0]
        ctr = (np.uint64(int(g)) << np.uint64(32)) | np.arange(R, dtype=np.uint64)
        w = philox_words(seed, iteration, ctr, STREAM_RAYS)
        fc[i] = vis[((w[0] * np.uint64(len(vis))) >> np.uint64(32)).astype(np.int64)]
        uxy[i, :, 0] = (w[1] >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0)
        uxy[i, :, 1] = (w[2] >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0)
    return fc, uxy

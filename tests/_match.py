"""Frontend::matchToMap's matching restated in numpy (test infrastructure for okvisgpu_match_to_map;
reference: okvis_frontend/src/Frontend.cpp:1299-1956, stereo_triangulation.cpp:30-112,
PinholeCamera.hpp:249-284 and 485-494).

  literal(scene)   the reference's loops as written: per keypoint a serial walk over the candidates
                   with a running best. Also returns the smallest margin of any floating-point
                   comparison it decided and the branch statistics the tests ask for.
  ordered(scene)   the parallel formulation: every candidate below the threshold is tested for
                   admissibility on its own; the match is the first minimum in order among the
                   admissible ones and the records are the strict prefix minima.
  build_scene(...) a scene (the arguments of okvisgpu.match_batch, cameras as dicts) on the ground
                   truth of a synthetic window.

A scene is a dict: poses, cameras (dicts: distortion, width, height, fu, fv, cu, cv, dist[8]),
extrinsics, landmarks, landmark_quality, landmark_use (or None), obs_begin, obs_pose, obs_camera,
obs_descriptor, obs_ray, imu_use, loop_closure, matching_threshold, job_camera, job_pass,
job_pose_prepare, job_pose_match, kp_begin, keypoint, descriptor, ray, ray_valid, landmark.

Margins: every floating-point comparison lhs ? rhs that decides a branch goes through Margin.lt /
.gt and records |lhs - rhs| / max(1, |lhs|, |rhs|). Comparisons of Hamming distances are integer
comparisons and cannot flip through rounding; neither can the comparison of two slots that both
still hold the initial score 1.0. A NaN operand (quality 0) decides "false" on every IEEE machine.
An acos argument within 1e-8 of +-1 counts as margin 0."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


class Margin:
    def __init__(self):
        self.worst = np.inf

    def note(self, lhs, rhs):
        if np.isnan(lhs) or np.isnan(rhs) or (np.isinf(lhs) and np.isinf(rhs)):
            return
        m = abs(lhs - rhs) / max(1.0, abs(lhs), abs(rhs))
        self.worst = min(self.worst, m)

    def lt(self, lhs, rhs):
        self.note(lhs, rhs)
        return lhs < rhs

    def gt(self, lhs, rhs):
        self.note(lhs, rhs)
        return lhs > rhs

    def acos(self, x):
        if abs(abs(x) - 1.0) < 1e-8:
            self.worst = 0.0
        with np.errstate(invalid="ignore"):
            return np.arccos(x)


def normalised(v):
    with np.errstate(invalid="ignore", over="ignore"):
        z = v @ v
        return v / np.sqrt(z) if z > 0 else v


def rotation(q):
    """Eigen's toRotationMatrix of the normalised quaternion (x, y, z, w)."""
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def compose(T_WS, T_SC):
    """T_WS T_SC as (C_WC, r_WC)."""
    C = rotation(T_WS[3:])
    return C @ rotation(T_SC[3:]), T_WS[:3] + C @ T_SC[:3]


def distort(cam, u):
    """distortion_.distort's point (radtan8's rho > 9 refusal is project_homogeneous')."""
    d, k = cam["distortion"], cam["dist"]
    u0, u1 = u
    if d == 0:
        return np.array([u0, u1])
    if d == 2:  # equidistant
        r = np.sqrt(u0 * u0 + u1 * u1)
        th = np.arctan(r)
        th2 = th * th
        thd = th * (1 + k[0] * th2 + k[1] * th2 ** 2 + k[2] * th2 ** 3 + k[3] * th2 ** 4)
        s = thd / r if r > 1e-8 else 1.0
        return np.array([s * u0, s * u1])
    mx, my, mxy = u0 * u0, u1 * u1, u0 * u1
    rho = mx + my
    if d == 1:  # radtan
        rad = k[0] * rho + k[1] * rho * rho
        return np.array([u0 + u0 * rad + 2 * k[2] * mxy + k[3] * (rho + 2 * mx),
                         u1 + u1 * rad + 2 * k[3] * mxy + k[2] * (rho + 2 * my)])
    rad = (1 + ((k[4] * rho + k[1]) * rho + k[0]) * rho) / (1 + ((k[7] * rho + k[6]) * rho + k[5]) * rho)
    return np.array([u0 * rad + 2 * k[2] * mxy + k[3] * (rho + 2 * mx),
                     u1 * rad + 2 * k[3] * mxy + k[2] * (rho + 2 * my)])


def project_homogeneous(cam, hp_C, M=None):
    """PinholeCamera::projectHomogeneous: (status, image point); status 'ok', 'outside', 'invalid',
    'behind'."""
    M = M or Margin()
    p = -hp_C[:3] if M.lt(hp_C[3], 0.0) else hp_C[:3]
    if M.lt(abs(p[2]), 1e-12):
        return "invalid", None
    rz = 1.0 / p[2]
    u = np.array([p[0] * rz, p[1] * rz])
    if cam["distortion"] == 3 and M.gt(u[0] * u[0] + u[1] * u[1], 9.0):
        return "invalid", None
    d = distort(cam, u)
    kp = np.array([cam["fu"] * d[0] + cam["cu"], cam["fv"] * d[1] + cam["cv"]])
    inside = not (M.lt(kp[0], 0.0) or M.lt(kp[1], 0.0)) and not (not M.lt(kp[0], cam["width"]) or
                                                                 not M.lt(kp[1], cam["height"]))
    if not inside:
        return "outside", kp
    return ("ok" if M.gt(p[2], 0.0) else "behind"), kp


def repr_threshold(cam, imu_use):
    f = 0.5 * (cam["fu"] + cam["fv"])
    return 3.0 + f * 0.06 if imu_use else 3.0 + f * 0.34


def prepare(s, M=None):
    """The candidate tables of every (job, landmark) (:1335-1508): dict of cand_n, cand_is3d, cand_obs,
    cand_projection, the slots' e0 / r0 [J, L, 3, 3], and kept [J, L] = the observations that were
    stored (more than 3: a slot was replaced)."""
    M = M or Margin()
    J, L = len(s["job_camera"]), len(s["landmarks"])
    out = {"cand_n": np.full((J, L), -1, np.int32), "cand_is3d": np.zeros((J, L), np.uint8),
           "cand_obs": np.full((J, L, 3), -1, np.int32), "cand_projection": np.zeros((J, L, 2)),
           "e0": np.zeros((J, L, 3, 3)), "r0": np.zeros((J, L, 3, 3)), "kept": np.zeros((J, L), np.int32)}
    loop = bool(s["loop_closure"])
    use = s.get("landmark_use")
    T_old = {}
    for j in range(J):
        c = int(s["job_camera"][j])
        cam = s["cameras"][c]
        thr = repr_threshold(cam, s["imu_use"])
        F = cam["fu"] + cam["fv"]
        C1, r1 = compose(s["job_pose_prepare"][j], s["extrinsics"][c])
        for l in range(L):
            if use is not None and not use[l]:
                continue
            hp = s["landmarks"][l]
            with np.errstate(all="ignore"):
                p_W = hp[:3] / hp[3]
            r_W = p_W - r1
            e_W = normalised(r_W)
            r = max(0.01, np.linalg.norm(r_W))
            hp_C = np.concatenate([C1.T @ (hp[:3] - r1 * hp[3]), hp[3:]])
            status, kp = project_homogeneous(cam, hp_C, M)
            if status in ("invalid", "behind"):
                continue
            if M.lt(kp[0], -thr) or M.lt(kp[1], -thr) or M.gt(kp[0], cam["width"] + thr) or \
                    M.gt(kp[1], cam["height"] + thr):
                continue
            quality = s["landmark_quality"][l]
            best = [1.0, 1.0, 1.0]
            slots = [-1, -1, -1]
            is3d, used, kept = False, 0, 0
            for o in range(int(s["obs_begin"][l + 1]) - 1, int(s["obs_begin"][l]) - 1, -1):
                key = (int(s["obs_pose"][o]), int(s["obs_camera"][o]))
                if key not in T_old:
                    T_old[key] = compose(s["poses"][key[0]], s["extrinsics"][key[1]])
                Co, ro = T_old[key]
                r_old = p_W - ro
                if not is3d:
                    with np.errstate(all="ignore"):
                        r_close = r_W - (np.float64(0.2) / F / np.float64(quality)) * r_old
                        cosA = normalised(r_W) @ normalised(r_close)
                    if M.gt(cosA, np.cos(10.0 / F)):
                        is3d = True
                cosV = e_W @ normalised(r_old)
                if M.lt(cosV, np.cos(0.6)) and not loop:
                    continue
                scale = abs(r - np.linalg.norm(r_old)) / r
                if M.gt(scale, 0.5) and not loop:
                    continue
                score = 0.5 * (M.acos(cosV) / 0.6 + scale / 0.5)
                worst, wi = 0.0, 0
                for n in range(3):
                    if best[n] == 1.0 and worst == 1.0:
                        continue  # two slots at the initial score: an exact comparison, false
                    if M.gt(best[n], worst):
                        worst, wi = best[n], n
                if M.lt(score, best[wi]):
                    best[wi], slots[wi] = score, o
                    out["e0"][j, l, wi] = Co @ normalised(s["obs_ray"][o])
                    out["r0"][j, l, wi] = ro
                    used = max(used, wi + 1)
                    kept += 1
            if used == 0:
                continue  # the deviation: the reference keeps one row of pool memory
            out["cand_n"][j, l] = used
            out["cand_is3d"][j, l] = is3d
            out["cand_obs"][j, l] = slots
            out["cand_projection"][j, l] = kp
            out["kept"][j, l] = kept
    return out


def hamming(a, b):
    """[n, 48] x [m, 48] uint8 -> [n, m] Hamming distances."""
    return POPCOUNT[a[:, None, :] ^ b[None, :, :]].sum(-1).astype(np.int32)


def triangulate_fast(p1, e1, p2, e2, sigma, M):
    """triangulation::triangulateFast: (point [3], valid, parallel)."""
    t12 = p2 - p1
    b = np.array([t12 @ e1, t12 @ e2])
    A00, A10 = e1 @ e1, e1 @ e2
    A01, A11 = -A10, -(e2 @ e2)
    det = A00 * A11 - A10 * A01
    invertible = M.gt(abs(det), 1e-12)
    fallback = not invertible
    if invertible:
        inv = 1.0 / det
        lam = np.array([A11 * inv * b[0] - A01 * inv * b[1], -A10 * inv * b[0] + A00 * inv * b[1]])
        fallback = M.lt(lam[0], 0.01) or M.lt(lam[1], 0.01)
    valid, parallel = True, False
    if fallback:
        parallel = True
        mid = (p1 + 0.5 * t12) + 40.0 * max(0.01, np.linalg.norm(t12)) * (e1 + e2)
    else:
        mid = ((lam[0] * e1 + p1) + (lam[1] * e2 + p2)) / 2.0
    n1, n2 = normalised(mid - p1), normalised(mid - p2)
    if M.lt(e1 @ n1, np.cos(2.6 * sigma)):
        valid = False
    if M.lt(e2 @ n2, np.cos(2.6 * sigma)):
        valid = False
    if not fallback and M.gt(n2 @ n1, np.cos(6.0 * sigma)):
        parallel = True
    return mid, valid, parallel


def admissible1(e0, r0, r1, e1, sigma, M):
    """Pass 1's tests of one slot (:1903-1939): (admissible, point, parallel)."""
    cos6 = np.cos(6.0 * sigma)
    if M.lt(e0 @ e1, cos6):
        et = normalised(r1 - r0)
        n0, n1 = normalised(np.cross(e0, et)), normalised(np.cross(e1, et))
        if M.lt(n0 @ n1, cos6):
            return False, None, False
        if M.gt(np.cross(e0, e1) @ normalised(n0 + n0), 0.0):
            return False, None, False
    pt, valid, parallel = triangulate_fast(r0, e0, r1, e1, sigma, M)
    if not valid:
        return False, None, False
    if M.lt(np.linalg.norm(pt - r0), 0.2) or M.lt(np.linalg.norm(pt - r1), 0.2):
        return False, None, False
    return True, pt, parallel


def _outputs(s):
    nk = int(s["kp_begin"][-1]) if len(s["kp_begin"]) else 0
    return {"match_landmark": np.full(nk, -1, np.int32), "match_distance": np.full(nk, -1, np.int32),
            "n_records": np.zeros(nk, np.int32), "record_repr_sum": np.zeros(nk), "point": np.zeros((nk, 4))}


def _job_tables(s, cand, j):
    """Slot descriptors of job j's candidates and the Hamming table of its keypoints against them."""
    k0, k1 = int(s["kp_begin"][j]), int(s["kp_begin"][j + 1])
    L = len(s["landmarks"])
    obs = np.maximum(cand["cand_obs"][j], 0).reshape(-1)
    if L == 0 or k1 == k0:
        return k0, k1, np.zeros((k1 - k0, L, 3), np.int32)
    desc = np.asarray(s["obs_descriptor"], np.uint8).reshape(-1, 48)[obs] if len(s["obs_pose"]) else \
        np.zeros((3 * L, 48), np.uint8)
    return k0, k1, hamming(np.asarray(s["descriptor"], np.uint8).reshape(-1, 48)[k0:k1], desc).reshape(k1 - k0, L, 3)


def _takes_part(s, k, job_pass):
    carried = int(s["landmark"][k])
    if carried >= 0 and not s["loop_closure"]:
        return False
    return bool(s["ray_valid"][k]) if job_pass == 1 else True


def literal(s):
    """The reference's loops. Returns the outputs of okvisgpu_match_to_map plus 'margin' and 'stats'."""
    M = Margin()
    cand = prepare(s, M)
    out = _outputs(s)
    J, L = len(s["job_camera"]), len(s["landmarks"])
    thr = float(s["matching_threshold"])
    stats = {"n_3d": [], "n_not3d": [], "accepted": [], "replaced": [], "point_not_of_match": 0,
             "carried_hits": 0}
    for j in range(J):
        c, job_pass = int(s["job_camera"][j]), int(s["job_pass"][j])
        cam = s["cameras"][c]
        k0, k1, dist = _job_tables(s, cand, j)
        is_cand = cand["cand_n"][j] > 0
        stats["n_3d"].append(int((is_cand & (cand["cand_is3d"][j] != 0)).sum()))
        stats["n_not3d"].append(int((is_cand & (cand["cand_is3d"][j] == 0)).sum()))
        stats["replaced"].append(int((cand["kept"][j] > 3).sum()))
        gate2 = repr_threshold(cam, s["imu_use"]) ** 2
        if job_pass == 1:
            C1, r1 = compose(s["job_pose_match"][j], s["extrinsics"][c])
            sigma = 1.0 / (0.5 * (cam["fu"] + cam["fv"]))
        for k in range(k0, k1):
            if not _takes_part(s, k, job_pass):
                continue
            best, match, count, rsum = thr, -1, 0, 0.0
            point, point_rec, match_rec = np.zeros(4), None, None
            carried = int(s["landmark"][k])
            if job_pass == 1:
                e1 = C1 @ normalised(s["ray"][k])
            for l in range(L):
                n = int(cand["cand_n"][j, l])
                if n <= 0 or bool(cand["cand_is3d"][j, l]) != (job_pass == 0):
                    continue
                if job_pass == 0:
                    rd = cand["cand_projection"][j, l] - s["keypoint"][k]
                    if M.gt(rd @ rd, gate2):
                        continue
                for d in range(n):
                    dk = float(dist[k - k0, l, d])
                    if not dk < best:
                        continue
                    if job_pass == 0:
                        best, match, count = dk, l, count + 1
                        rsum += np.sqrt(rd @ rd)
                        continue
                    ok, pt, parallel = admissible1(cand["e0"][j, l, d], cand["r0"][j, l, d], r1, e1, sigma, M)
                    if not ok:
                        continue
                    if l == carried:
                        count += 1
                        stats["carried_hits"] += 1
                        break
                    best, match, count, match_rec = dk, l, count + 1, (l, d)
                    if not parallel:
                        point, point_rec = np.array([pt[0], pt[1], pt[2], 1.0]), (l, d)
            out["match_landmark"][k] = match
            out["match_distance"][k] = int(best) if match >= 0 else -1
            out["n_records"][k] = count
            out["record_repr_sum"][k] = rsum
            out["point"][k] = point
            if point_rec is not None and point_rec != match_rec:
                stats["point_not_of_match"] += 1
        stats["accepted"].append(int((out["match_landmark"][k0:k1] >= 0).sum()))
    out.update({k: cand[k] for k in ("cand_n", "cand_is3d", "cand_obs", "cand_projection")})
    out["margin"] = M.worst
    out["stats"] = stats
    return out


def ordered(s):
    """The parallel formulation: admissibility of every candidate below the threshold on its own, then
    first minimum in order and strict prefix minima."""
    M = Margin()
    cand = prepare(s, M)
    out = _outputs(s)
    J, L = len(s["job_camera"]), len(s["landmarks"])
    thr = float(s["matching_threshold"])
    for j in range(J):
        c, job_pass = int(s["job_camera"][j]), int(s["job_pass"][j])
        cam = s["cameras"][c]
        k0, k1, dist = _job_tables(s, cand, j)
        gate2 = repr_threshold(cam, s["imu_use"]) ** 2
        slot_ok = (np.arange(3)[None, :] < cand["cand_n"][j][:, None]) & \
            ((cand["cand_is3d"][j] != 0) == (job_pass == 0))[:, None]  # [L, 3]
        if job_pass == 1:
            C1, r1 = compose(s["job_pose_match"][j], s["extrinsics"][c])
            sigma = 1.0 / (0.5 * (cam["fu"] + cam["fv"]))
        for k in range(k0, k1):
            if not _takes_part(s, k, job_pass):
                continue
            d = dist[k - k0].astype(np.float64)  # [L, 3]
            adm = slot_ok & (d < thr)
            rd = np.zeros(L)
            if job_pass == 0 and L:
                diff = cand["cand_projection"][j] - s["keypoint"][k]
                rd2 = (diff * diff).sum(-1)
                adm &= ~(rd2 > gate2)[:, None]
                rd = np.sqrt(rd2)
            pts, par = {}, {}
            if job_pass == 1:
                e1 = C1 @ normalised(s["ray"][k])
                for l, sl in zip(*np.nonzero(adm)):
                    ok, pt, parallel = admissible1(cand["e0"][j, l, sl], cand["r0"][j, l, sl], r1, e1, sigma, M)
                    adm[l, sl] = ok
                    pts[(l, sl)], par[(l, sl)] = pt, parallel
            carried = int(s["landmark"][k]) if job_pass == 1 else -1
            seq = np.where(adm, d, np.inf)
            count_carried = 0
            if carried >= 0 and L:
                own = seq[carried].copy()
                seq[carried] = np.inf  # the carried landmark never lowers the best
            flat = seq.reshape(-1)
            before = np.minimum(thr, np.concatenate([[np.inf], np.minimum.accumulate(flat)[:-1]])) if len(flat) else flat
            rec = flat < before
            if carried >= 0 and L:
                count_carried = int((own < before.reshape(L, 3)[carried][0]).any())
            idx = np.flatnonzero(rec)
            out["n_records"][k] = len(idx) + count_carried
            if len(idx):
                m = int(np.argmin(flat))  # the first minimum in order
                out["match_landmark"][k] = m // 3
                out["match_distance"][k] = int(flat[m])
                if job_pass == 0:
                    out["record_repr_sum"][k] = sum(rd[i // 3] for i in idx)
                else:
                    nonpar = [i for i in idx if not par[(i // 3, i % 3)]]
                    if nonpar:
                        out["point"][k] = [*pts[(nonpar[-1] // 3, nonpar[-1] % 3)], 1.0]
    out.update({k: cand[k] for k in ("cand_n", "cand_is3d", "cand_obs", "cand_projection")})
    return out


INT_KEYS = ("match_landmark", "match_distance", "n_records", "cand_n", "cand_is3d", "cand_obs")
REAL_KEYS = ("cand_projection", "record_repr_sum", "point")


def worst_relative(got, ref):
    """max |got - ref| / max(1, |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


# ------------------------------------------------------------------------------------------ scenes
def box_plus(T, dr, da):
    """T with its position moved by dr and its rotation by the small angle da (left-multiplied)."""
    half = 0.5 * np.asarray(da)
    dq = np.array([*half, np.sqrt(max(0.0, 1.0 - half @ half))])
    x1, y1, z1, w1 = dq
    x2, y2, z2, w2 = T[3:]
    q = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                  w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    return np.concatenate([T[:3] + dr, q / np.linalg.norm(q)])


def flip_bits(rng, desc, n):
    d = np.unpackbits(desc.copy())
    d[rng.choice(384, size=n, replace=False)] ^= 1
    return np.packbits(d)


def build_scene(gt_poses, gt_landmarks, extrinsics, cameras, obs_pose, obs_landmark, obs_camera, seed,
                loop_closure=False, passes=(0, 1), imu_use=True, distractors=0.3):
    """A matching scene on a window's ground truth. The map is all poses but the last (with the
    observations from them), the current frame the last pose: prepared at a perturbed pose, matched at
    a less perturbed one. One job per camera and pass, all over the same keypoints per camera."""
    rng = np.random.default_rng(seed)
    n_pose, L = len(gt_poses) - 1, len(gt_landmarks)
    cur = gt_poses[-1]
    # observations of the map in (landmark; frame, camera) order
    keep = np.flatnonzero(np.asarray(obs_pose) < n_pose)
    order = keep[np.lexsort((np.asarray(obs_camera)[keep], np.asarray(obs_pose)[keep], np.asarray(obs_landmark)[keep]))]
    o_lm, o_pose, o_cam = (np.asarray(a)[order].astype(np.int32) for a in (obs_landmark, obs_pose, obs_camera))
    obs_begin = np.concatenate([[0], np.cumsum(np.bincount(o_lm, minlength=L))]).astype(np.int32)
    lm_desc = rng.integers(0, 256, size=(L, 48), dtype=np.uint8)
    obs_desc = np.array([flip_bits(rng, lm_desc[l], int(rng.integers(0, 41))) for l in o_lm], np.uint8).reshape(-1, 48)
    obs_ray = np.zeros((len(order), 3))
    for i, (l, p, c) in enumerate(zip(o_lm, o_pose, o_cam)):
        C, r = compose(gt_poses[p], extrinsics[c])
        e = C.T @ (gt_landmarks[l][:3] / gt_landmarks[l][3] - r)
        obs_ray[i] = e / e[2] + np.array([*rng.normal(0.0, 1.0 / cameras[c]["fu"], 2), 0.0])
    # both landmark classes: half the map at a quality that makes every observation's test pass, half
    # at one that makes none pass
    quality = np.where(rng.random(L) < 0.5, 0.5, 1e-4)
    use = None
    if loop_closure:
        use = (np.arange(L) % 3 == 0).astype(np.uint8)
    kps, descs, rays, valid, carried, begin = [], [], [], [], [], [0]
    job_camera, job_pass = [], []
    per_camera = {}
    for c, cam in enumerate(cameras):
        C, r = compose(cur, extrinsics[c])
        kp, de, ra, va, ca = [], [], [], [], []
        for l in range(L):
            p_C = C.T @ (gt_landmarks[l][:3] / gt_landmarks[l][3] - r)
            status, px = project_homogeneous(cam, np.array([*p_C, 1.0]))
            if status != "ok":
                continue
            kp.append(px + rng.normal(0.0, 1.0, 2))
            de.append(flip_bits(rng, lm_desc[l], int(rng.integers(0, 41))))
            ra.append(p_C / p_C[2] + np.array([*rng.normal(0.0, 0.3 / cam["fu"], 2), 0.0]))
            va.append(rng.random() < 0.95)
            u = rng.random()
            if loop_closure:
                ca.append(l if u < 0.5 else (int(rng.integers(0, L)) if u < 0.6 else -1))
            else:
                ca.append(l if u < 0.1 else -1)
        for _ in range(int(distractors * len(kp))):
            kp.append(np.array([rng.uniform(0, cam["width"]), rng.uniform(0, cam["height"])]))
            de.append(rng.integers(0, 256, size=48, dtype=np.uint8))
            ra.append(np.array([*rng.uniform(-0.5, 0.5, 2), 1.0]))
            va.append(True)
            ca.append(-1)
        perm = rng.permutation(len(kp))
        per_camera[c] = [np.array(a)[perm] for a in (kp, de, ra, va, ca)]
    for job_p in passes:
        for c in range(len(cameras)):
            kp, de, ra, va, ca = per_camera[c]
            kps.append(kp.reshape(-1, 2)); descs.append(de.reshape(-1, 48)); rays.append(ra.reshape(-1, 3))
            valid.append(va.reshape(-1)); carried.append(ca.reshape(-1))
            begin.append(begin[-1] + len(kp))
            job_camera.append(c)
            job_pass.append(job_p)
    J = len(job_camera)
    prepared = box_plus(cur, rng.normal(0.0, 0.03, 3), rng.normal(0.0, 0.005, 3))
    matched = box_plus(cur, rng.normal(0.0, 0.003, 3), rng.normal(0.0, 0.0005, 3))
    return {"poses": np.ascontiguousarray(gt_poses[:n_pose]), "cameras": cameras,
            "extrinsics": np.ascontiguousarray(extrinsics), "landmarks": np.ascontiguousarray(gt_landmarks),
            "landmark_quality": quality, "landmark_use": use, "obs_begin": obs_begin, "obs_pose": o_pose,
            "obs_camera": o_cam, "obs_descriptor": obs_desc, "obs_ray": obs_ray, "imu_use": imu_use,
            "loop_closure": loop_closure, "matching_threshold": 60.0,
            "job_camera": np.array(job_camera, np.int32), "job_pass": np.array(job_pass, np.int32),
            "job_pose_prepare": np.tile(prepared, (J, 1)), "job_pose_match": np.tile(matched, (J, 1)),
            "kp_begin": np.array(begin, np.int32), "keypoint": np.concatenate(kps), "descriptor": np.concatenate(descs),
            "ray": np.concatenate(rays), "ray_valid": np.concatenate(valid).astype(np.uint8),
            "landmark": np.concatenate(carried).astype(np.int32)}


def pinhole(distortion=0, dist=(), f=400.0, width=640, height=480):
    return {"distortion": distortion, "width": width, "height": height, "fu": f, "fv": f * 1.01, "cu": width / 2 - 3.5,
            "cv": height / 2 + 2.25, "dist": list(dist) + [0.0] * (8 - len(dist))}


def toy_world(n_poses, n_landmarks, cameras, seed, full_landmarks=0):
    """Ground truth for build_scene without a synthetic window: poses along a gently curving path
    looking down +z, cameras side by side, landmarks 3..10 m in front; every landmark is observed from
    a few (pose, camera) pairs that see it, the first `full_landmarks` from camera 0 of every pose.
    Returns (poses, landmarks, extrinsics, obs_pose, obs_landmark, obs_camera)."""
    rng = np.random.default_rng(seed)
    poses = np.array([box_plus(np.array([0.12 * i, 0.02 * np.sin(0.7 * i), 0.03 * i, 0, 0, 0, 1.0]), np.zeros(3),
                               np.array([0.004 * i, -0.006 * i, 0.003 * i])) for i in range(n_poses)])
    extrinsics = np.array([box_plus(np.array([0.11 * c, 0.01 * c, 0.0, 0, 0, 0, 1.0]), np.zeros(3),
                                    np.array([0.002 * c, 0.003 * c, -0.001 * c])) for c in range(len(cameras))])
    landmarks = np.column_stack([rng.uniform(-2.0, 3.0, n_landmarks), rng.uniform(-1.5, 1.5, n_landmarks),
                                 rng.uniform(3.0, 10.0, n_landmarks), np.ones(n_landmarks)])
    landmarks[:full_landmarks, :3] = [0.6, 0.1, 6.0] + rng.uniform(-0.3, 0.3, (full_landmarks, 3))
    op, ol, oc = [], [], []
    for l in range(n_landmarks):
        for p in range(n_poses - 1):
            for c, cam in enumerate(cameras):
                if l < full_landmarks:
                    if c != 0:
                        continue
                elif rng.random() > 0.35:
                    continue
                C, r = compose(poses[p], extrinsics[c])
                status, _ = project_homogeneous(cam, np.array([*(C.T @ (landmarks[l, :3] - r)), 1.0]))
                if status == "ok":
                    op.append(p); ol.append(l); oc.append(c)
    return poses, landmarks, extrinsics, np.array(op, np.int32), np.array(ol, np.int32), np.array(oc, np.int32)


def append_landmark(s, hp, quality, obs, use=1):
    """A copy of the scene with one more landmark (the highest id): obs = [(pose, camera, descriptor
    [48], ray [3])] in (pose, camera) order."""
    t = dict(s)
    t["landmarks"] = np.vstack([np.asarray(s["landmarks"]).reshape(-1, 4), np.asarray(hp, np.float64)[None]])
    t["landmark_quality"] = np.append(s["landmark_quality"], quality)
    if s.get("landmark_use") is not None:
        t["landmark_use"] = np.append(s["landmark_use"], use).astype(np.uint8)
    t["obs_begin"] = np.append(s["obs_begin"], s["obs_begin"][-1] + len(obs)).astype(np.int32)
    t["obs_pose"] = np.append(s["obs_pose"], [o[0] for o in obs]).astype(np.int32)
    t["obs_camera"] = np.append(s["obs_camera"], [o[1] for o in obs]).astype(np.int32)
    t["obs_descriptor"] = np.vstack([np.asarray(s["obs_descriptor"], np.uint8).reshape(-1, 48)] +
                                    [np.asarray(o[2], np.uint8)[None] for o in obs])
    t["obs_ray"] = np.vstack([np.asarray(s["obs_ray"]).reshape(-1, 3)] + [np.asarray(o[3], np.float64)[None] for o in obs])
    return t


def with_jobs(s, jobs):
    """A copy of the scene with its jobs replaced: jobs = [(camera, pass, keypoint indices of the scene,
    pose_prepare, pose_match)]."""
    t = dict(s)
    begin = [0]
    for _, _, idx, _, _ in jobs:
        begin.append(begin[-1] + len(idx))
    sel = np.concatenate([np.asarray(j[2], np.int64) for j in jobs]) if jobs else np.zeros(0, np.int64)
    for k in ("keypoint", "descriptor", "ray", "ray_valid", "landmark"):
        t[k] = np.ascontiguousarray(np.asarray(s[k])[sel])
    t["job_camera"] = np.array([j[0] for j in jobs], np.int32)
    t["job_pass"] = np.array([j[1] for j in jobs], np.int32)
    t["job_pose_prepare"] = np.array([j[3] for j in jobs], np.float64).reshape(-1, 7)
    t["job_pose_match"] = np.array([j[4] for j in jobs], np.float64).reshape(-1, 7)
    t["kp_begin"] = np.array(begin, np.int32)
    return t


def sub_scene(s, jobs):
    """The scene restricted to the given jobs (in the given order)."""
    t = dict(s)
    begin, parts = [0], {k: [] for k in ("keypoint", "descriptor", "ray", "ray_valid", "landmark")}
    for j in jobs:
        a, b = int(s["kp_begin"][j]), int(s["kp_begin"][j + 1])
        begin.append(begin[-1] + b - a)
        for k in parts:
            parts[k].append(s[k][a:b])
    for k in ("job_camera", "job_pass", "job_pose_prepare", "job_pose_match"):
        t[k] = np.ascontiguousarray(np.asarray(s[k])[list(jobs)])
    t["kp_begin"] = np.array(begin, np.int32)
    for k, v in parts.items():
        t[k] = np.concatenate(v) if v else s[k][:0]
    return t


def job_rows(s, out, j):
    """Job j's part of every output, as a dict of arrays."""
    a, b = int(s["kp_begin"][j]), int(s["kp_begin"][j + 1])
    r = {k: out[k][a:b] for k in ("match_landmark", "match_distance", "n_records", "record_repr_sum", "point")}
    r.update({k: out[k][j] for k in ("cand_n", "cand_is3d", "cand_obs", "cand_projection")})
    return r

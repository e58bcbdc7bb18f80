"""Builds tests/native/libks_lanecheck.so (host build of the kernel source, TEST ONLY)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from kinovagrasping_amd.sim import SOLVER_ITERATIONS

HERE = Path(__file__).resolve().parent / "native"
CSRC = Path(__file__).resolve().parents[1] / "kinovagrasping_amd" / "csrc"
dp = C.POINTER(C.c_double)


def lanecheck_lib(multi_geom: bool = False):
    """multi_geom: the kernel source compiled with -DKS_MULTI_GEOM (the topology capacities of libkinova_sim_mg.so)"""
    so, src = HERE / ("libks_lanecheck_mg.so" if multi_geom else "libks_lanecheck.so"), HERE / "ks_lanecheck.cpp"
    deps = [src] + sorted(CSRC.glob("*.h"))
    if not so.exists() or any(d.stat().st_mtime > so.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DKS_GJK_COUNT_IDS"] + (["-DKS_MULTI_GEOM"] if multi_geom else []) + ["-o", str(so), str(src)])
    L = C.CDLL(str(so))
    L.lc_create.restype = C.c_void_p
    L.lc_create.argtypes = [C.c_char_p, C.c_size_t]
    L.lc_destroy.argtypes = [C.c_void_p]
    L.lc_substep.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, dp, C.c_int, C.POINTER(C.c_int), dp]
    L.lc_substep_mass.argtypes = L.lc_substep.argtypes + [C.c_double]
    L.lc_env_step.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, dp, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int), dp]
    L.lc_reset_obs.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int), dp]
    L.lc_get_warm.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.lc_put_warm.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.lc_set_warm.argtypes = [C.c_void_p, C.c_int]
    L.lc_gjk_ids_out_of_range.restype = C.c_long
    _obs_entry(L)
    return L


def _obs_entry(L):
    ip = C.POINTER(C.c_int)
    L.lc_create.restype = C.c_void_p
    L.lc_create.argtypes = [C.c_char_p, C.c_size_t]
    L.lc_destroy.argtypes = [C.c_void_p]
    L.lc_build_obs.argtypes = [C.c_void_p, C.c_int, dp, dp, C.c_int, dp, ip, dp, ip, dp]
    L.lc_build_obs.restype = None


def obs_lane_lib(root: Path, so: Path):
    """the observation entry alone (-DKS_LC_OBS_ONLY) of the tree under `root` (tests/native/ks_lanecheck.cpp and kinovagrasping_amd/csrc
    below it) -> so.  tests/test_obs_cpu.py builds copies of the source with one deliberate error each this way."""
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DKS_LC_OBS_ONLY", "-o", str(so), str(Path(root) / "tests" / "native" / "ks_lanecheck.cpp")])
    L = C.CDLL(str(so))
    _obs_entry(L)
    return L


def build_obs_lane(L, h, prec, snap, rays, part=-1, obs=None, written=None):
    """lc_build_obs of one snapshot [105] and its rays [17]: (obs [82], writes per slot [82], reward, the lift test twice - bit 0 build_obs' own, bit 1 object_lifted's -, info [3]); obs / written
    given: filled on top of what they hold (the four parts one after the other)"""
    obs = np.full(82, np.nan) if obs is None else obs
    written = np.zeros(82, dtype=np.int32) if written is None else written
    rew, done, info = C.c_double(0), C.c_int(0), np.zeros(3)
    L.lc_build_obs(h, prec, P(np.ascontiguousarray(snap, dtype=np.float64)), P(np.ascontiguousarray(rays, dtype=np.float64)), part, P(obs),
                   written.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rew), C.byref(done), P(info))
    return obs, written, rew.value, done.value, info


def P(a):
    return a.ctypes.data_as(dp)


class Lane:
    """one lane of the kernel source on the CPU, fp32 or fp64"""

    def __init__(self, blob: bytes, prec: int, iters: int = SOLVER_ITERATIONS, multi_geom: bool = False):
        self.L = lanecheck_lib(multi_geom)
        self.h = self.L.lc_create(blob, len(blob))
        assert self.h, "lc_create failed (see stderr)"
        self.prec, self.iters = prec, iters

    def substep(self, qpos, qvel, warm, ctrl, hq, obj_mass=0.0):
        """obj_mass > 0: the env's object mass (ks_set_env_params of the product)"""
        a, b, c = (np.array(x, dtype=np.float64) for x in (qpos, qvel, warm))
        nc = C.c_int(0)
        ncm = self.L.lc_ncon_max()
        con = np.zeros(ncm * 20)
        args = (self.h, self.prec, P(a), P(b), P(c), P(np.array(ctrl, dtype=np.float64)), P(np.array(hq, dtype=np.float64)), self.iters, C.byref(nc), P(con))
        st = self.L.lc_substep_mass(*args, C.c_double(obj_mass)) if obj_mass > 0 else self.L.lc_substep(*args)
        return a, b, c, nc.value, con.reshape(ncm, 20), st

    def env_step(self, qpos, qvel, warm, hq, act, frame_skip=15):
        a, b, c = (np.array(x, dtype=np.float64) for x in (qpos, qvel, warm))
        obs, rays, rew, done = np.zeros(82), np.zeros(17), C.c_double(0), C.c_int(0)
        st = self.L.lc_env_step(self.h, self.prec, P(a), P(b), P(c), P(np.array(hq, dtype=np.float64)), P(np.array(act, dtype=np.float64)),
                                frame_skip, self.iters, P(obs), C.byref(rew), C.byref(done), P(rays))
        return a, b, c, obs, rew.value, bool(done.value), rays, st

    def reset_obs(self, qpos0, hq):
        a, b, c = np.array(qpos0, dtype=np.float64), np.zeros(15), np.zeros(15)
        obs, rays, rew, done = np.zeros(82), np.zeros(17), C.c_double(0), C.c_int(0)
        self.L.lc_reset_obs(self.h, self.prec, P(a), P(b), P(c), P(np.array(hq, dtype=np.float64)), P(obs), C.byref(rew), C.byref(done), P(rays))
        return obs, rays

    # ---- pair memory (fp32 lane): what the lane remembers of its hull pairs' last queries (ks_core.h: PairWarm)
    def set_warm(self, on: bool):
        """on: remember from one substep() to the next, starting from nothing; off: cold queries"""
        self.L.lc_set_warm(self.h, int(on))

    def get_warm(self):
        out = np.zeros(self.L.lc_warm_words(), dtype=np.uint32)
        self.L.lc_get_warm(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out

    def put_warm(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        assert w.size == self.L.lc_warm_words()
        self.L.lc_put_warm(self.h, w.ctypes.data_as(C.POINTER(C.c_uint32)))

    def ids_out_of_range(self):
        """remembered simplex ids beyond the pair's hull tables that gjk_distance met since the last call (process-wide counter)"""
        return int(self.L.lc_gjk_ids_out_of_range())

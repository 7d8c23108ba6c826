"""Thin Python host side over the C ABI (include/vigo.h).

PyTorch is used for device memory, streams and torch.distributed only; every computation on
the hot path happens inside libvigo_hip.so.  All tensor arguments must be contiguous CUDA
(= HIP) tensors of the dtype the header states; nothing here touches the CPU oracle.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import VigoParams

PREC_F64 = 0
PREC_F32 = 1
PREC_F64_FAST = 2
ASTAR_FOUND, ASTAR_NOT_FOUND, ASTAR_DEFERRED, ASTAR_PATH_TOO_LONG = 0, 1, 2, 3   # vigo_astar_search's out_status
GUIDE_OK, GUIDE_DEFERRED = 0, 1                                                  # vigo_guide_assign's out_status
REGUIDE_DONE, REGUIDE_SEARCH_FAILED, REGUIDE_NOT_REQUIRED, REGUIDE_DEFERRED, REGUIDE_SKIPPED = 0, 1, 2, 3, 4   # vigo_rebound_reguide's out_status
PATHS_OK, PATHS_FAILED, PATHS_DEFERRED = 0, 1, 2                                 # vigo_collision_segs' / vigo_path_search's out_status
SEED_OK, SEED_NO_SPACING, SEED_GOAL_OCCUPIED, SEED_TOO_SHORT, SEED_DEFERRED, SEED_BAD_INPUT = 0, 1, 2, 3, 4, 5   # vigo_seed_paths' out_status
FINISH_OK, FINISH_CAPACITY, FINISH_INVALID_N = 0, 1, 2   # vigo_traj_finish's out_status
VALID_STATIC, VALID_DYNAMIC, VALID_BAD_COUNT = 1, 2, 4   # vigo_traj_validate's out_status bits (include/vigo_validate.h)
VALIDATE_BY_TIME, VALIDATE_BY_INDEX = 0, 1               # ... and its rules

# lbfgs.hpp:20-80 status codes worth naming
LBFGS_CONVERGENCE = 0
LBFGS_STOP = 1
LBFGS_ALREADY_MINIMIZED = 2
_LB_BASE = -1024
_LB_NAMES = [
    "LBFGSERR_UNKNOWNERROR", "LBFGSERR_LOGICERROR", "LBFGSERR_CANCELED", "LBFGSERR_INVALID_N",
    "LBFGSERR_INVALID_MEMSIZE", "LBFGSERR_INVALID_GEPSILON", "LBFGSERR_INVALID_TESTPERIOD",
    "LBFGSERR_INVALID_DELTA", "LBFGSERR_INVALID_MINSTEP", "LBFGSERR_INVALID_MAXSTEP",
    "LBFGSERR_INVALID_FDECCOEFF", "LBFGSERR_INVALID_SCURVCOEFF", "LBFGSERR_INVALID_XTOL",
    "LBFGSERR_INVALID_MAXLINESEARCH", "LBFGSERR_OUTOFINTERVAL", "LBFGSERR_INCORRECT_TMINMAX",
    "LBFGSERR_ROUNDING_ERROR", "LBFGSERR_MINIMUMSTEP", "LBFGSERR_MAXIMUMSTEP",
    "LBFGSERR_MAXIMUMLINESEARCH", "LBFGSERR_MAXIMUMITERATION", "LBFGSERR_WIDTHTOOSMALL",
    "LBFGSERR_INVALIDPARAMETERS", "LBFGSERR_INCREASEGRADIENT",
]
LBFGS_CODES = {name: _LB_BASE + i for i, name in enumerate(_LB_NAMES)}
LBFGSERR_ROUNDING_ERROR = LBFGS_CODES["LBFGSERR_ROUNDING_ERROR"]
LBFGSERR_MAXIMUMLINESEARCH = LBFGS_CODES["LBFGSERR_MAXIMUMLINESEARCH"]
LBFGSERR_MAXIMUMITERATION = LBFGS_CODES["LBFGSERR_MAXIMUMITERATION"]


class VigoError(RuntimeError):
    pass


def default_params() -> VigoParams:
    p = VigoParams()
    _lib.load().vigo_default_params(C.byref(p))
    return p


def _ptr(t: Optional[torch.Tensor], dtype, name: str, device=None):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (the C ABI takes device pointers)")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, handle is bound to {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return C.c_void_p(t.data_ptr())


def _shape(t: Optional[torch.Tensor], want, name: str):
    """the kernels index by these extents: a tensor of another shape is an out-of-range read on the device"""
    if t is None:
        return
    got = tuple(t.shape)
    if len(got) != len(want) or any(w is not None and g != w for g, w in zip(got, want)):
        raise ValueError(f"{name}: shape {got}, expected {tuple('*' if w is None else w for w in want)}")


@dataclass
class SolveResult:
    ctrl: torch.Tensor      # [B,N,3] optData_.controlPoints after optimize() (last evaluated point)
    x: torch.Tensor         # [B,N-6,3] the vector lbfgs_optimize returns
    status: torch.Tensor    # [B] int32, lbfgs.hpp:20-80
    fx: torch.Tensor        # [B]
    iters: torch.Tensor     # [B] int32
    evals: torch.Tensor     # [B] int32


class Vigo:
    """One vigo_handle_t bound to one GPU (one per process/rank)."""

    def __init__(self, device: int = 0, params: Optional[VigoParams] = None, precision: int = PREC_F64):
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise VigoError("no HIP device visible: the ViGO hot path has no CPU fallback")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        rc = self._lib.vigo_create(C.byref(h), device)
        if rc != 0:
            raise VigoError(f"vigo_create failed with {rc}")
        self._h = h
        self.params = params if params is not None else default_params()
        self.set_params(self.params)
        self.set_precision(precision)
        self._grid_meta = None

    # ---- lifecycle -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.vigo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.vigo_last_error(self._h)
            raise VigoError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_params(self, p: VigoParams):
        self._check(self._lib.vigo_set_params(self._h, C.byref(p)), "vigo_set_params")
        self.params = p

    def set_precision(self, precision: int):
        self._check(self._lib.vigo_set_precision(self._h, precision), "vigo_set_precision")
        self.precision = precision

    def use_current_stream(self):
        """Bind launches to torch's current stream on this device."""
        s = torch.cuda.current_stream(self.device)
        self._check(self._lib.vigo_set_stream(self._h, C.c_void_p(s.cuda_stream)), "vigo_set_stream")

    # ---- voxel map ---------------------------------------------------------------------
    def set_grid(self, voxels: torch.Tensor, origin, res: float):
        """voxels: uint8 [nx,ny,nz] on the GPU (bit0 inflated-occupied, bit1 unknown, bit2 occupied)."""
        nx, ny, nz = voxels.shape
        o = (C.c_double * 3)(*origin)
        self._check(self._lib.vigo_set_grid(self._h, nx, ny, nz, o, float(res),
                                            _ptr(voxels, torch.uint8, "voxels", self.device)), "vigo_set_grid")
        self._grid_meta = (nx, ny, nz, tuple(float(v) for v in origin), float(res))

    def set_grid_host(self, voxels, origin, res: float):
        """vigo_set_grid_host: voxels a C-contiguous uint8 numpy array [nx,ny,nz] in host memory (staged and packed)."""
        if voxels.dtype.name != "uint8" or voxels.ndim != 3 or not voxels.flags["C_CONTIGUOUS"]:
            raise ValueError("voxels: expected a C-contiguous uint8 array [nx,ny,nz]")
        nx, ny, nz = voxels.shape
        o = (C.c_double * 3)(*origin)
        self._check(self._lib.vigo_set_grid_host(self._h, nx, ny, nz, o, float(res), C.c_void_p(voxels.ctypes.data)),
                    "vigo_set_grid_host")
        self._grid_meta = (nx, ny, nz, tuple(float(v) for v in origin), float(res))

    def inflate_grid(self, voxels: torch.Tensor, rx: int, ry: int, rz: int) -> torch.Tensor:
        """in place: bit0 := OR of bit2 over the (2rx+1)(2ry+1)(2rz+1) voxel box"""
        nx, ny, nz = voxels.shape
        self._check(self._lib.vigo_inflate_grid(self._h, nx, ny, nz, _ptr(voxels, torch.uint8, "voxels", self.device), rx, ry, rz),
                    "vigo_inflate_grid")
        return voxels

    def pack_grid(self, voxels: torch.Tensor) -> torch.Tensor:
        """Pack a byte grid into the snapshot format (int32 tensor) for an RCCL broadcast."""
        nx, ny, nz = voxels.shape
        nbytes = self._lib.vigo_grid_packed_bytes(nx, ny, nz)
        packed = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
        self._check(self._lib.vigo_pack_grid(self._h, nx, ny, nz, _ptr(voxels, torch.uint8, "voxels", self.device),
                                             C.c_void_p(packed.data_ptr())), "vigo_pack_grid")
        return packed

    def set_grid_packed(self, packed: torch.Tensor, dims, origin, res: float):
        nx, ny, nz = dims
        if packed.numel() * 4 != self._lib.vigo_grid_packed_bytes(nx, ny, nz):
            raise ValueError("packed grid has the wrong size for these dims")
        o = (C.c_double * 3)(*origin)
        self._check(self._lib.vigo_set_grid_packed(self._h, nx, ny, nz, o, float(res),
                                                   _ptr(packed, torch.int32, "packed", self.device)),
                    "vigo_set_grid_packed")
        self._grid_meta = (nx, ny, nz, tuple(float(v) for v in origin), float(res))

    def set_metric_bounds(self, bmin, bmax):
        self._check(self._lib.vigo_set_metric_bounds(self._h, (C.c_double * 3)(*bmin), (C.c_double * 3)(*bmax)),
                    "vigo_set_metric_bounds")

    @staticmethod
    def _int3(v, name: str):
        v = [int(x) for x in v]
        if len(v) != 3:
            raise ValueError(f"{name}: expected three integers")
        return (C.c_int32 * 3)(*v)

    def update_grid_region(self, lo, voxels: torch.Tensor, inflate_r=None):
        """vigo_update_grid_region: the box of voxels.shape at lo written into the snapshot in place, stream-ordered.
        voxels: uint8 [n0,n1,n2] on the GPU.  inflate_r None: raw (bits 0..2 of the bytes); (rx,ry,rz): bit 0 is ignored and
        plane 0 is re-inflated from the occupied plane on the box grown by r.  A field built by build_esdf is stale afterwards:
        build it again, or build it with build_esdf(tracked=True) once and call update_esdf() after the region updates — the
        boxes are collected in the handle's pending box and the field is refreshed for work that follows the change."""
        if voxels.dim() != 3:
            raise ValueError("voxels: expected [n0,n1,n2]")
        r = None if inflate_r is None else self._int3(inflate_r, "inflate_r")
        p = _ptr(voxels, torch.uint8, "voxels", self.device) if voxels.numel() else C.c_void_p(voxels.data_ptr() or 1)
        self._check(self._lib.vigo_update_grid_region(self._h, self._int3(lo, "lo"), self._int3(voxels.shape, "n"), p, r),
                    "vigo_update_grid_region")

    def update_grid_region_host(self, lo, voxels, inflate_r=None):
        """vigo_update_grid_region_host: the same from a C-contiguous uint8 numpy array [n0,n1,n2] (staged; synchronises)."""
        if voxels.dtype.name != "uint8" or voxels.ndim != 3 or not voxels.flags["C_CONTIGUOUS"]:
            raise ValueError("voxels: expected a C-contiguous uint8 array [n0,n1,n2]")
        r = None if inflate_r is None else self._int3(inflate_r, "inflate_r")
        self._check(self._lib.vigo_update_grid_region_host(self._h, self._int3(lo, "lo"), self._int3(voxels.shape, "n"),
                                                           C.c_void_p(voxels.ctypes.data or 1), r), "vigo_update_grid_region_host")

    def get_grid_packed(self) -> torch.Tensor:
        """vigo_get_grid_packed: a copy of the handle's current snapshot (int32 tensor, the format of pack_grid)."""
        if self._grid_meta is None:
            raise VigoError("get_grid_packed before set_grid")
        nx, ny, nz = self._grid_meta[:3]
        packed = torch.empty(self._lib.vigo_grid_packed_bytes(nx, ny, nz) // 4, dtype=torch.int32, device=self.device)
        self._check(self._lib.vigo_get_grid_packed(self._h, C.c_void_p(packed.data_ptr())), "vigo_get_grid_packed")
        return packed

    def query_points(self, pts: torch.Tensor, which: int = 0) -> torch.Tensor:
        _shape(pts, (None, 3), "pts")
        q = pts.shape[0]
        out = torch.empty(q, dtype=torch.uint8, device=self.device)
        self._check(self._lib.vigo_query_points(self._h, which, q, _ptr(pts, torch.float64, "pts", self.device),
                                                C.c_void_p(out.data_ptr())), "vigo_query_points")
        return out

    def guides_unknown(self, guide_pv: torch.Tensor) -> torch.Tensor:
        _shape(guide_pv, (None, 6), "guide_pv")
        g = guide_pv.shape[0]
        out = torch.empty(g, dtype=torch.uint8, device=self.device)
        if g:
            self._check(self._lib.vigo_guides_unknown(self._h, g, _ptr(guide_pv, torch.float64, "guide_pv", self.device),
                                                      C.c_void_p(out.data_ptr())), "vigo_guides_unknown")
        return out

    # ---- cost / solve ------------------------------------------------------------------
    def _solve_ptrs(self, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights):
        B, N, three = ctrl.shape
        if three != 3:
            raise ValueError("ctrl must be [B,N,3]")
        if guide_off is not None and guide_off.numel() != B * N + 1:
            raise ValueError("guide_off must have B*N+1 entries")
        if obs_off is not None and obs_off.numel() != B + 1:
            raise ValueError("obs_off must have B+1 entries")
        if weights is not None and tuple(weights.shape) != (B, 4):
            raise ValueError("weights must be [B,4]")
        _shape(guide_pv, (None, 6), "guide_pv")
        _shape(obs, (None, 9), "obs")
        if guide_unk is not None and guide_pv is not None and guide_unk.numel() != guide_pv.shape[0]:
            raise ValueError("guide_unk must have one entry per guide pair")
        n_shared = 0
        if obs is not None and obs_off is None:
            n_shared = obs.shape[0]
        d = self.device
        return (B, N, _ptr(ctrl, torch.float64, "ctrl", d), _ptr(guide_off, torch.int32, "guide_off", d),
                _ptr(guide_pv, torch.float64, "guide_pv", d), _ptr(guide_unk, torch.uint8, "guide_unk", d),
                _ptr(obs_off, torch.int32, "obs_off", d), _ptr(obs, torch.float64, "obs", d), n_shared,
                _ptr(weights, torch.float64, "weights", d))

    def check_lists(self, B: int, N: int, guide_off=None, n_pairs: int = 0, obs_off=None, n_obs: int = 0) -> int:
        """vigo_check_lists: number of CSR violations in guide_off [B*N+1] / obs_off [B+1] (0 = safe to pass)."""
        if guide_off is not None and guide_off.numel() != B * N + 1:
            raise ValueError("guide_off must have B*N+1 entries")
        if obs_off is not None and obs_off.numel() != B + 1:
            raise ValueError("obs_off must have B+1 entries")
        rc = self._lib.vigo_check_lists(self._h, B, N, _ptr(guide_off, torch.int32, "guide_off", self.device), int(n_pairs),
                                        _ptr(obs_off, torch.int32, "obs_off", self.device), int(n_obs))
        if rc < 0:
            self._check(rc, "vigo_check_lists")
        return rc

    def cost_grad(self, ctrl, guide_off=None, guide_pv=None, guide_unk=None, obs_off=None, obs=None,
                  weights=None, want_terms=True):
        """vigo_cost_grad: returns (cost[B], grad[B,N-6,3], terms[B,4] or None)."""
        B, N, pc, po, ppv, pu, poo, pob, ns, pw = self._solve_ptrs(ctrl, guide_off, guide_pv, guide_unk,
                                                                    obs_off, obs, weights)
        cost = torch.empty(B, dtype=torch.float64, device=self.device)
        grad = torch.empty(B, max(N - 6, 0), 3, dtype=torch.float64, device=self.device)
        terms = torch.empty(B, 4, dtype=torch.float64, device=self.device) if want_terms else None
        self._check(self._lib.vigo_cost_grad(self._h, B, N, pc, po, ppv, pu, poo, pob, ns, pw,
                                             C.c_void_p(cost.data_ptr()), C.c_void_p(grad.data_ptr()),
                                             C.c_void_p(terms.data_ptr()) if want_terms else None), "vigo_cost_grad")
        return cost, grad, terms

    def optimize(self, ctrl, guide_off=None, guide_pv=None, guide_unk=None, obs_off=None, obs=None,
                 weights=None, inplace=False, out: Optional[SolveResult] = None) -> SolveResult:
        """vigo_optimize.  ctrl is cloned unless inplace=True (the C ABI updates it in place)."""
        _shape(ctrl, (None, None, 3), "ctrl")
        if ctrl.shape[1] < 7:
            raise VigoError(f"vigo_optimize needs N >= 7 control points (got {ctrl.shape[1]}): VIGO_ERR_UNSUPPORTED_N")
        work = ctrl if inplace else ctrl.clone()
        B, N, pc, po, ppv, pu, poo, pob, ns, pw = self._solve_ptrs(work, guide_off, guide_pv, guide_unk,
                                                                    obs_off, obs, weights)
        d = self.device
        if out is not None:
            # a caller-owned result is written by the kernel: wrong extents are out-of-range device writes
            _shape(out.x, (B, N - 6, 3), "out.x")
            for name in ("status", "iters", "evals", "fx"):
                _shape(getattr(out, name), (B,), f"out.{name}")
            _ptr(out.x, torch.float64, "out.x", d)
            _ptr(out.fx, torch.float64, "out.fx", d)
            for name in ("status", "iters", "evals"):
                _ptr(getattr(out, name), torch.int32, f"out.{name}", d)
        if out is None:
            out = SolveResult(
                ctrl=work,
                x=torch.empty(B, N - 6, 3, dtype=torch.float64, device=self.device),
                status=torch.empty(B, dtype=torch.int32, device=self.device),
                fx=torch.empty(B, dtype=torch.float64, device=self.device),
                iters=torch.empty(B, dtype=torch.int32, device=self.device),
                evals=torch.empty(B, dtype=torch.int32, device=self.device),
            )
        else:
            out.ctrl = work
        self._check(self._lib.vigo_optimize(self._h, B, N, pc, po, ppv, pu, poo, pob, ns, pw,
                                            C.c_void_p(out.x.data_ptr()), C.c_void_p(out.status.data_ptr()),
                                            C.c_void_p(out.fx.data_ptr()), C.c_void_p(out.iters.data_ptr()),
                                            C.c_void_p(out.evals.data_ptr())), "vigo_optimize")
        return out

    # ---- the rebound loop between two A* calls ---------------------------------------------
    # vigo_rebound_state_t as int32 columns: status, solve_first, fail_count, gate_static, gate_dynamic, rounds,
    # lbfgs_status, n_seg, then 2 * VIGO_MAX_COLLISION_SEGS segment indices
    REBOUND_MAX_SEGS = 48
    REBOUND_STATE_INTS = 8 + 2 * 48
    RB_ACTIVE, RB_DONE, RB_NEEDS_HOST = 0, 1, 2

    def rebound_rounds(self, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights, gate_dt, state,
                       max_rounds=4, not_check_ratio=0.0):
        """vigo_rebound_rounds: ctrl [B,N,3], weights [B,4] and state [B, REBOUND_STATE_INTS] (int32) are updated in place."""
        B, N, pc, po, ppv, pu, poo, pob, ns, pw = self._solve_ptrs(ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights)
        if weights is None:
            raise ValueError("weights [B,4] are required (the loop doubles them per trajectory)")
        _shape(state, (B, self.REBOUND_STATE_INTS), "state")
        self._check(self._lib.vigo_rebound_rounds(self._h, B, N, pc, po, ppv, pu, poo, pob, ns, pw, float(gate_dt),
                                                  float(not_check_ratio), int(max_rounds),
                                                  _ptr(state, torch.int32, "state", self.device)), "vigo_rebound_rounds")

    # ---- mixed control-point counts: rows of Ns control points, n_pts[b] of them trajectory b's -------------------
    def _mixed_ptrs(self, n_pts, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights):
        """the uniform entries' pointers (ctrl [B,Ns,3], guide_off [B*Ns+1]) and n_pts int32 [B].  The counts are device
        data: the kernels check them per trajectory (include/vigo.h, "mixed control-point counts")."""
        _shape(ctrl, (None, None, 3), "ctrl")
        B, Ns = ctrl.shape[0], ctrl.shape[1]
        if n_pts is not None:
            _shape(n_pts, (B,), "n_pts")
        return self._solve_ptrs(ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights) + (
            _ptr(n_pts, torch.int32, "n_pts", self.device),)

    def cost_grad_mixed(self, n_pts, ctrl, guide_off=None, guide_pv=None, guide_unk=None, obs_off=None, obs=None,
                        weights=None, want_terms=True, out=None):
        """vigo_cost_grad_mixed: returns (cost[B], grad[B,Ns-6,3], terms[B,4] or None); rows of grad beyond
        n_pts[b] - 6 are not written.  out: caller-owned (cost, grad, terms) to write into."""
        B, Ns, pc, po, ppv, pu, poo, pob, ns, pw, pn = self._mixed_ptrs(n_pts, ctrl, guide_off, guide_pv, guide_unk,
                                                                         obs_off, obs, weights)
        if out is not None:
            cost, grad, terms = out
            _shape(cost, (B,), "out cost"); _shape(grad, (B, max(Ns - 6, 0), 3), "out grad"); _shape(terms, (B, 4), "out terms")
            for t, name in ((cost, "out cost"), (grad, "out grad"), (terms, "out terms")):
                _ptr(t, torch.float64, name, self.device)
        else:
            cost = torch.zeros(B, dtype=torch.float64, device=self.device)
            grad = torch.zeros(B, max(Ns - 6, 0), 3, dtype=torch.float64, device=self.device)
            terms = torch.zeros(B, 4, dtype=torch.float64, device=self.device) if want_terms else None
        self._check(self._lib.vigo_cost_grad_mixed(self._h, B, Ns, pn, pc, po, ppv, pu, poo, pob, ns, pw,
                                                   C.c_void_p(cost.data_ptr()), C.c_void_p(grad.data_ptr()),
                                                   C.c_void_p(terms.data_ptr()) if terms is not None else None),
                    "vigo_cost_grad_mixed")
        return cost, grad, terms

    def optimize_mixed(self, n_pts, ctrl, guide_off=None, guide_pv=None, guide_unk=None, obs_off=None, obs=None,
                       weights=None, inplace=False, out: Optional[SolveResult] = None) -> SolveResult:
        """vigo_optimize_mixed.  ctrl [B,Ns,3] is cloned unless inplace=True; x is [B,Ns-6,3], its rows beyond
        n_pts[b] - 6 (and every output of a trajectory with a bad count but its status) are not written: zeros, or
        what the caller's `out` held."""
        work = ctrl if inplace else ctrl.clone()
        B, Ns, pc, po, ppv, pu, poo, pob, ns, pw, pn = self._mixed_ptrs(n_pts, work, guide_off, guide_pv, guide_unk,
                                                                         obs_off, obs, weights)
        d = self.device
        if out is not None:
            _shape(out.x, (B, max(Ns - 6, 0), 3), "out.x")
            for name in ("status", "iters", "evals", "fx"):
                _shape(getattr(out, name), (B,), f"out.{name}")
            _ptr(out.x, torch.float64, "out.x", d)
            _ptr(out.fx, torch.float64, "out.fx", d)
            for name in ("status", "iters", "evals"):
                _ptr(getattr(out, name), torch.int32, f"out.{name}", d)
            out.ctrl = work
        else:
            out = SolveResult(
                ctrl=work,
                x=torch.zeros(B, max(Ns - 6, 0), 3, dtype=torch.float64, device=d),
                status=torch.zeros(B, dtype=torch.int32, device=d),
                fx=torch.zeros(B, dtype=torch.float64, device=d),
                iters=torch.zeros(B, dtype=torch.int32, device=d),
                evals=torch.zeros(B, dtype=torch.int32, device=d),
            )
        self._check(self._lib.vigo_optimize_mixed(self._h, B, Ns, pn, pc, po, ppv, pu, poo, pob, ns, pw,
                                                  C.c_void_p(out.x.data_ptr()), C.c_void_p(out.status.data_ptr()),
                                                  C.c_void_p(out.fx.data_ptr()), C.c_void_p(out.iters.data_ptr()),
                                                  C.c_void_p(out.evals.data_ptr())), "vigo_optimize_mixed")
        return out

    def rebound_rounds_mixed(self, n_pts, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, weights, gate_dt, state,
                             max_rounds=4, not_check_ratio=0.0):
        """vigo_rebound_rounds_mixed: ctrl [B,Ns,3], weights [B,4] and state [B, REBOUND_STATE_INTS] are updated in place."""
        B, Ns, pc, po, ppv, pu, poo, pob, ns, pw, pn = self._mixed_ptrs(n_pts, ctrl, guide_off, guide_pv, guide_unk,
                                                                         obs_off, obs, weights)
        if weights is None:
            raise ValueError("weights [B,4] are required (the loop doubles them per trajectory)")
        _shape(state, (B, self.REBOUND_STATE_INTS), "state")
        self._check(self._lib.vigo_rebound_rounds_mixed(self._h, B, Ns, pn, pc, po, ppv, pu, poo, pob, ns, pw, float(gate_dt),
                                                        float(not_check_ratio), int(max_rounds),
                                                        _ptr(state, torch.int32, "state", self.device)),
                    "vigo_rebound_rounds_mixed")

    # ---- spline fit, evaluation and gates -----------------------------------------------
    def bspline_fit(self, points, conds=None, ts=None):
        """bspline::parameterizeToBspline for a batch: points [B,K,3] (+ conds [B,4,3]) -> ctrl [B,K+2,3]"""
        _shape(points, (None, None, 3), "points")
        B, K, _ = points.shape
        _shape(conds, (B, 4, 3), "conds")
        ts = float(self.params.ts_ctrl if ts is None else ts)
        out = torch.empty(B, K + 2, 3, dtype=torch.float64, device=self.device)
        self._check(self._lib.vigo_bspline_fit(self._h, B, K, ts, _ptr(points, torch.float64, "points", self.device),
                                               _ptr(conds, torch.float64, "conds", self.device),
                                               C.c_void_p(out.data_ptr())), "vigo_bspline_fit")
        return out

    def bspline_fit_mixed(self, points, n_fit, Ns, conds=None, status=None, ts=None, out=None):
        """vigo_bspline_fit_mixed: points [T,point_stride,3] f64, of which the first n_fit[t] (i32 [T]) rows are path t's
        (+ conds [T,4,3], status i32 [T]: only paths of status 0 are fitted) -> (ctrl [T,Ns,3], n_pts i32 [T]), the input
        of optimize_mixed.  Rows of ctrl beyond n_fit[t] + 2, and the whole row of a path that is not fitted (n_pts 0),
        are not written: zeros, or what the caller's out = (ctrl, n_pts) held."""
        _shape(points, (None, None, 3), "points")
        T, stride, _ = points.shape
        Ns = int(Ns)
        _shape(n_fit, (T,), "n_fit")
        _shape(status, (T,), "status")
        _shape(conds, (T, 4, 3), "conds")
        ts = float(self.params.ts_ctrl if ts is None else ts)
        d = self.device
        if out is not None:
            ctrl, n_pts = out
            _shape(ctrl, (T, Ns, 3), "out ctrl"); _shape(n_pts, (T,), "out n_pts")
            _ptr(ctrl, torch.float64, "out ctrl", d); _ptr(n_pts, torch.int32, "out n_pts", d)
        else:
            ctrl = torch.zeros(T, max(Ns, 0), 3, dtype=torch.float64, device=d)
            n_pts = torch.zeros(T, dtype=torch.int32, device=d)
        self._check(self._lib.vigo_bspline_fit_mixed(self._h, T, Ns, ts, _ptr(n_fit, torch.int32, "n_fit", d),
                                                     _ptr(status, torch.int32, "status", d),
                                                     _ptr(points, torch.float64, "points", d), stride,
                                                     _ptr(conds, torch.float64, "conds", d),
                                                     C.c_void_p(ctrl.data_ptr()), C.c_void_p(n_pts.data_ptr())),
                    "vigo_bspline_fit_mixed")
        return ctrl, n_pts

    def bspline_eval(self, ctrl, times, deriv=0):
        _shape(ctrl, (None, None, 3), "ctrl")
        B, N, _ = ctrl.shape
        T = times.numel()
        out = torch.empty(B, T, 3, dtype=torch.float64, device=self.device)
        self._check(self._lib.vigo_bspline_eval(self._h, B, N, _ptr(ctrl, torch.float64, "ctrl", self.device), deriv, T,
                                                _ptr(times, torch.float64, "times", self.device),
                                                C.c_void_p(out.data_ptr())), "vigo_bspline_eval")
        return out

    def traj_collision(self, ctrl, dt):
        _shape(ctrl, (None, None, 3), "ctrl")
        B, N, _ = ctrl.shape
        flag = torch.empty(B, dtype=torch.uint8, device=self.device)
        first = torch.empty(B, dtype=torch.int32, device=self.device)
        self._check(self._lib.vigo_traj_collision(self._h, B, N, _ptr(ctrl, torch.float64, "ctrl", self.device),
                                                  float(dt), C.c_void_p(flag.data_ptr()),
                                                  C.c_void_p(first.data_ptr())), "vigo_traj_collision")
        return flag, first

    def traj_finish(self, ctrl, limits, sample_dt, S_cap, n_pts=None, out=None, want_max=True, want_vel=True):
        """vigo_traj_finish: the end of a plan for ctrl [B,Ns,3] f64 (row b holds n_pts[b] control points, i32 [B]; None:
        Ns each) with limits [B,2] f64 = max_vel, max_acc -> dict of factor f64[B] (linearFactor_), max f64[B,2] (maxV,
        maxA; None without want_max), n i32[B] (samples of the `t <= duration; t += sample_dt` loop), pos f64[B,S_cap,3],
        vel f64[B,S_cap,3] (at i * sample_dt; None without want_vel), status i32[B] (FINISH_*).  Sample rows beyond n, and
        every row of an INVALID_N trajectory, are not written: zeros, or what the caller's out = (pos, vel) held."""
        _shape(ctrl, (None, None, 3), "ctrl")
        B, Ns, _ = ctrl.shape
        S_cap = int(S_cap)
        _shape(limits, (B, 2), "limits")
        _shape(n_pts, (B,), "n_pts")
        d = self.device
        if out is not None:
            pos, vel = out
            _shape(pos, (B, S_cap, 3), "out pos"); _ptr(pos, torch.float64, "out pos", d)
            if vel is not None:
                _shape(vel, (B, S_cap, 3), "out vel"); _ptr(vel, torch.float64, "out vel", d)
        else:
            pos = torch.zeros(B, max(S_cap, 0), 3, dtype=torch.float64, device=d)
            vel = torch.zeros(B, max(S_cap, 0), 3, dtype=torch.float64, device=d) if want_vel else None
        factor = torch.zeros(B, dtype=torch.float64, device=d)
        mx = torch.zeros(B, 2, dtype=torch.float64, device=d) if want_max else None
        n = torch.zeros(B, dtype=torch.int32, device=d)
        status = torch.zeros(B, dtype=torch.int32, device=d)
        self._check(self._lib.vigo_traj_finish(self._h, B, Ns, _ptr(n_pts, torch.int32, "n_pts", d),
                                               _ptr(ctrl, torch.float64, "ctrl", d), _ptr(limits, torch.float64, "limits", d),
                                               float(sample_dt), S_cap, C.c_void_p(factor.data_ptr()),
                                               None if mx is None else C.c_void_p(mx.data_ptr()), C.c_void_p(n.data_ptr()),
                                               C.c_void_p(pos.data_ptr()), None if vel is None else C.c_void_p(vel.data_ptr()),
                                               C.c_void_p(status.data_ptr())), "vigo_traj_finish")
        return {"factor": factor, "max": mx, "n": n, "pos": pos, "vel": vel, "status": status}

    def traj_validate(self, ctrl, dt, n_pts=None, not_check_ratio=0.0, rule=0, obs_off=None, obs=None, want_list=True, out=None,
                      want_pos=True, want_dyn=True):
        """vigo_traj_validate (include/vigo_validate.h): are the held plans ctrl [B,Ns,3] f64 (row b holds n_pts[b] control
        points, i32 [B]; None: Ns each) still valid on the current map -> dict of status i32[B] (VALID_* bits, 0 = valid),
        first i32[B] (first colliding static sample or -1), pos f64[B,3] (its position; None without want_pos),
        dyn_first i32[B] (first sample inside an obstacle or -1; None without want_dyn), invalid i32[B] and n_invalid
        i32[1] (the rows with a status, ascending, and their number; None without want_list).  rule 0: the static check
        covers t <= (1 - not_check_ratio) * duration, rule 1: the samples k < (1 - not_check_ratio) * S.  Rows of pos
        without a static hit and entries of invalid beyond n_invalid are not written: zeros, or what the caller's
        out = (pos, invalid) held.  Stream-ordered, no host round trip."""
        _shape(ctrl, (None, None, 3), "ctrl")
        B, Ns, _ = ctrl.shape
        _shape(n_pts, (B,), "n_pts")
        _shape(obs, (None, 9), "obs")
        if obs_off is not None and obs_off.numel() != B + 1:
            raise ValueError("obs_off must have B+1 entries")
        d = self.device
        pos = torch.zeros(B, 3, dtype=torch.float64, device=d) if want_pos else None
        invalid = torch.zeros(B, dtype=torch.int32, device=d) if want_list else None
        if out is not None:
            pos, invalid = out
            if pos is not None:
                _shape(pos, (B, 3), "out pos"); _ptr(pos, torch.float64, "out pos", d)
            if invalid is not None:
                _shape(invalid, (B,), "out invalid"); _ptr(invalid, torch.int32, "out invalid", d)
        status = torch.zeros(B, dtype=torch.int32, device=d)
        first = torch.zeros(B, dtype=torch.int32, device=d)
        dyn = torch.zeros(B, dtype=torch.int32, device=d) if want_dyn else None
        n_invalid = torch.zeros(1, dtype=torch.int32, device=d) if invalid is not None else None
        ns = obs.shape[0] if (obs is not None and obs_off is None) else 0
        opt = lambda t: None if t is None else C.c_void_p(t.data_ptr() or 1)       # (an empty tensor has no address: B == 0 reads nothing)
        self._check(self._lib.vigo_traj_validate(self._h, B, Ns, _ptr(n_pts, torch.int32, "n_pts", d), _ptr(ctrl, torch.float64, "ctrl", d),
                                                 float(dt), float(not_check_ratio), int(rule), _ptr(obs_off, torch.int32, "obs_off", d),
                                                 _ptr(obs, torch.float64, "obs", d), ns, opt(status), opt(first), opt(pos), opt(dyn),
                                                 opt(invalid), opt(n_invalid)), "vigo_traj_validate")
        return {"status": status, "first": first, "pos": pos, "dyn_first": dyn, "invalid": invalid, "n_invalid": n_invalid}

    def traj_dynamic_collision(self, ctrl, dt, obs_off=None, obs=None):
        _shape(ctrl, (None, None, 3), "ctrl")
        B, N, _ = ctrl.shape
        _shape(obs, (None, 9), "obs")
        if obs_off is not None and obs_off.numel() != B + 1:
            raise ValueError("obs_off must have B+1 entries")
        flag = torch.empty(B, dtype=torch.uint8, device=self.device)
        ns = obs.shape[0] if (obs is not None and obs_off is None) else 0
        self._check(self._lib.vigo_traj_dynamic_collision(
            self._h, B, N, _ptr(ctrl, torch.float64, "ctrl", self.device), float(dt),
            _ptr(obs_off, torch.int32, "obs_off", self.device), _ptr(obs, torch.float64, "obs", self.device), ns,
            C.c_void_p(flag.data_ptr())), "vigo_traj_dynamic_collision")
        return flag

    def ctrl_occupancy(self, ctrl):
        _shape(ctrl, (None, None, 3), "ctrl")
        B, N, _ = ctrl.shape
        pt = torch.empty(B, N, dtype=torch.uint8, device=self.device)
        line = torch.empty(B, N, dtype=torch.uint8, device=self.device)
        self._check(self._lib.vigo_ctrl_occupancy(self._h, B, N, _ptr(ctrl, torch.float64, "ctrl", self.device),
                                                  C.c_void_p(pt.data_ptr()), C.c_void_p(line.data_ptr())),
                    "vigo_ctrl_occupancy")
        return pt, line

    # ---- corridor checker ---------------------------------------------------------------
    def minsnap(self, waypoints, corridor=None, conds=None, deg=7, diff=4, cont=4, vel=1.0, corridor_res=8.0):
        """polyTrajSolver::solve for a batch of paths: waypoints [T,W,3] (+ corridor [T,W-1], conds [T,4,3])
        -> (coeffs [T,W-1,3,deg+1], knots [T,W], status [T])"""
        _shape(waypoints, (None, None, 3), "waypoints")
        T, W, _ = waypoints.shape
        _shape(corridor, (T, W - 1), "corridor")
        _shape(conds, (T, 4, 3), "conds")
        coeffs = torch.zeros(T, W - 1, 3, deg + 1, dtype=torch.float64, device=self.device)
        knots = torch.zeros(T, W, dtype=torch.float64, device=self.device)
        status = torch.full((T,), -99, dtype=torch.int32, device=self.device)
        self._check(self._lib.vigo_minsnap(self._h, T, W, deg, diff, cont, float(vel), float(corridor_res),
                                           _ptr(waypoints, torch.float64, "waypoints", self.device),
                                           _ptr(corridor, torch.float64, "corridor", self.device),
                                           _ptr(conds, torch.float64, "conds", self.device),
                                           C.c_void_p(coeffs.data_ptr()), C.c_void_p(knots.data_ptr()),
                                           C.c_void_p(status.data_ptr())), "vigo_minsnap")
        return coeffs, knots, status

    def corridor_check(self, coeffs, n_samp, delT, box, map_res):
        """coeffs [S,3,deg+1] f64, n_samp [S] i32, delT [S] f64 -> (flag u8[S], first i32[S], count i32[S])."""
        _shape(coeffs, (None, 3, None), "coeffs")
        S, three, d1 = coeffs.shape
        _shape(n_samp, (S,), "n_samp")
        _shape(delT, (S,), "delT")
        flag = torch.empty(S, dtype=torch.uint8, device=self.device)
        first = torch.empty(S, dtype=torch.int32, device=self.device)
        count = torch.empty(S, dtype=torch.int32, device=self.device)
        self._check(self._lib.vigo_corridor_check(
            self._h, S, d1 - 1, _ptr(coeffs, torch.float64, "coeffs", self.device),
            _ptr(n_samp, torch.int32, "n_samp", self.device), _ptr(delT, torch.float64, "delT", self.device),
            (C.c_double * 3)(*box), float(map_res), C.c_void_p(flag.data_ptr()), C.c_void_p(first.data_ptr()),
            C.c_void_p(count.data_ptr())), "vigo_corridor_check")
        return flag, first, count

    def traj_corridor_check(self, seg_off, coeffs, knots, delT, endpoint, box, map_res, nonfinite_collides=False):
        """vigo_traj_corridor_check: T whole trajectories, seg_off [T+1] i32 (CSR over the S segments), coeffs [S,3,deg+1]
        f64, knots [S+T] f64, delT [T] f64, endpoint [T,3] f64 -> (status i32[T], n i32[T], flag u8[T], first i32[T],
        count i32[T], seg u8[S])"""
        _shape(seg_off, (None,), "seg_off")
        T = seg_off.shape[0] - 1
        if T < 0:
            raise ValueError("seg_off: needs T + 1 >= 1 entries")
        _shape(coeffs, (None, 3, None), "coeffs")
        S, _, d1 = coeffs.shape
        _shape(knots, (S + T,), "knots")
        _shape(delT, (T,), "delT")
        _shape(endpoint, (T, 3), "endpoint")
        d = self.device
        status = torch.empty(T, dtype=torch.int32, device=d)
        n = torch.empty(T, dtype=torch.int32, device=d)
        flag = torch.empty(T, dtype=torch.uint8, device=d)
        first = torch.empty(T, dtype=torch.int32, device=d)
        count = torch.empty(T, dtype=torch.int32, device=d)
        seg = torch.empty(S, dtype=torch.uint8, device=d)
        self._check(self._lib.vigo_traj_corridor_check(
            self._h, T, S, d1 - 1, _ptr(seg_off, torch.int32, "seg_off", d), _ptr(coeffs, torch.float64, "coeffs", d),
            _ptr(knots, torch.float64, "knots", d), _ptr(delT, torch.float64, "delT", d),
            _ptr(endpoint, torch.float64, "endpoint", d), (C.c_double * 3)(*box), float(map_res), 1 if nonfinite_collides else 0,
            C.c_void_p(status.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(flag.data_ptr()), C.c_void_p(first.data_ptr()),
            C.c_void_p(count.data_ptr()), C.c_void_p(seg.data_ptr())), "vigo_traj_corridor_check")
        return status, n, flag, first, count, seg

    def traj_point_check(self, seg_off, coeffs, knots, delT, endpoint):
        """vigo_traj_point_check: traj_corridor_check's arguments and outputs, the test being the point lookup of
        polyTrajOccMap (bits 0 and 1 of the pose's voxel both set) -> (status, n, flag, first, count, seg)"""
        _shape(seg_off, (None,), "seg_off")
        T = seg_off.shape[0] - 1
        if T < 0:
            raise ValueError("seg_off: needs T + 1 >= 1 entries")
        _shape(coeffs, (None, 3, None), "coeffs")
        S, _, d1 = coeffs.shape
        _shape(knots, (S + T,), "knots")
        _shape(delT, (T,), "delT")
        _shape(endpoint, (T, 3), "endpoint")
        d = self.device
        status = torch.empty(T, dtype=torch.int32, device=d)
        n = torch.empty(T, dtype=torch.int32, device=d)
        flag = torch.empty(T, dtype=torch.uint8, device=d)
        first = torch.empty(T, dtype=torch.int32, device=d)
        count = torch.empty(T, dtype=torch.int32, device=d)
        seg = torch.empty(S, dtype=torch.uint8, device=d)
        self._check(self._lib.vigo_traj_point_check(
            self._h, T, S, d1 - 1, _ptr(seg_off, torch.int32, "seg_off", d), _ptr(coeffs, torch.float64, "coeffs", d),
            _ptr(knots, torch.float64, "knots", d), _ptr(delT, torch.float64, "delT", d),
            _ptr(endpoint, torch.float64, "endpoint", d), C.c_void_p(status.data_ptr()), C.c_void_p(n.data_ptr()),
            C.c_void_p(flag.data_ptr()), C.c_void_p(first.data_ptr()), C.c_void_p(count.data_ptr()),
            C.c_void_p(seg.data_ptr())), "vigo_traj_point_check")
        return status, n, flag, first, count, seg

    def seed_paths(self, seg_off, coeffs, knots, duration, dt0, control_point_distance, max_path_length, prev_in_seed=None,
                   prev_in_fit=None, max_tries=16, point_cap=256):
        """vigo_seed_paths: the seed-path stage between polyTrajOccMap and bsplineTraj for T trajectories.  seg_off [T+1]
        i32, coeffs [S,3,deg+1] f64, knots [S+T] f64 as traj_point_check; duration, dt0, control_point_distance,
        max_path_length, prev_in_seed, prev_in_fit [T] f64 (the prev arrays default to zeros) -> dict of status i32[T]
        (SEED_*), tries i32[T], dt f64[T], final_time f64[T], seed_n i32[T], seed f64[T,point_cap,3], fit_n i32[T],
        fit f64[T,point_cap,3], prev_seed f64[T], prev_fit f64[T].  Outputs start zeroed: a SEED_DEFERRED trajectory
        keeps zeros."""
        _shape(seg_off, (None,), "seg_off")
        T = seg_off.shape[0] - 1
        if T < 0:
            raise ValueError("seg_off: needs T + 1 >= 1 entries")
        _shape(coeffs, (None, 3, None), "coeffs")
        S, _, d1 = coeffs.shape
        _shape(knots, (S + T,), "knots")
        d = self.device
        if prev_in_seed is None:
            prev_in_seed = torch.zeros(T, dtype=torch.float64, device=d)
        if prev_in_fit is None:
            prev_in_fit = torch.zeros(T, dtype=torch.float64, device=d)
        per = {"duration": duration, "dt0": dt0, "control_point_distance": control_point_distance,
               "max_path_length": max_path_length, "prev_in_seed": prev_in_seed, "prev_in_fit": prev_in_fit}
        for name, a in per.items():
            _shape(a, (T,), name)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=d)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=d)
        out = {"status": i32(T), "tries": i32(T), "dt": f64(T), "final_time": f64(T), "seed_n": i32(T),
               "seed": f64(T, point_cap, 3), "fit_n": i32(T), "fit": f64(T, point_cap, 3), "prev_seed": f64(T), "prev_fit": f64(T)}
        self._check(self._lib.vigo_seed_paths(
            self._h, T, S, d1 - 1, _ptr(seg_off, torch.int32, "seg_off", d), _ptr(coeffs, torch.float64, "coeffs", d),
            _ptr(knots, torch.float64, "knots", d), *[_ptr(a, torch.float64, name, d) for name, a in per.items()],
            int(max_tries), int(point_cap), *[C.c_void_p(out[k].data_ptr()) for k in
                                              ("status", "tries", "dt", "final_time", "seed_n", "seed", "fit_n", "fit", "prev_seed", "prev_fit")]),
            "vigo_seed_paths")
        return out

    def astar_search(self, start, end, step, pool, min_height, max_height, max_expansions=1 << 20, path_cap=256, want_stats=True):
        """vigo_astar_search: Q searches of the facade's host A* on the handle's grid -> (status int32 [Q], len int32 [Q],
        path f64 [Q,path_cap,3], stats int32 [Q,3] or None); status ASTAR_FOUND / NOT_FOUND / DEFERRED / PATH_TOO_LONG"""
        _shape(start, (None, 3), "start")
        Q = start.shape[0]
        _shape(end, (Q, 3), "end")
        d = self.device
        status = torch.full((Q,), -1, dtype=torch.int32, device=d)
        length = torch.zeros(Q, dtype=torch.int32, device=d)
        path = torch.zeros((Q, int(path_cap), 3), dtype=torch.float64, device=d)
        stats = torch.zeros((Q, 3), dtype=torch.int32, device=d) if want_stats else None
        self._check(self._lib.vigo_astar_search(
            self._h, Q, _ptr(start, torch.float64, "start", d), _ptr(end, torch.float64, "end", d), float(step),
            (C.c_int32 * 3)(*[int(v) for v in pool]), float(min_height), float(max_height), int(max_expansions), int(path_cap),
            C.c_void_p(status.data_ptr()), C.c_void_p(length.data_ptr()), C.c_void_p(path.data_ptr()),
            C.c_void_p(stats.data_ptr()) if want_stats else None), "vigo_astar_search")
        return status, length, path, stats

    def _rows_call(self, name, n_pts, ctrl):
        """(entry, its name, leading arguments) of a prologue entry: the uniform one, or with n_pts (int32 [B], device) its
        _mixed form, where ctrl is [B,Ns,3] and the counts are device data the kernels check per trajectory"""
        _shape(ctrl, (None, None, 3), "ctrl")
        B, N = ctrl.shape[0], ctrl.shape[1]
        if n_pts is None:
            return getattr(self._lib, name), name, (self._h, B, N)
        _shape(n_pts, (B,), "n_pts")
        return getattr(self._lib, name + "_mixed"), name + "_mixed", (self._h, B, N, _ptr(n_pts, torch.int32, "n_pts", self.device))

    def guide_assign(self, ctrl, seg_off, seg, path_off, path, pair_cap, want_unknown=True, fill=None, _n_pts=None):
        """vigo_guide_assign: the prologue's guide assignment for B trajectories (ctrl f64 [B,N,3]; seg_off int32 [B+1], seg int32
        [S,2], path_off int32 [S+1], path f64 [P,3]) -> (guide_off int32 [B*N+1], guide_pv f64 [pair_cap,6], guide_unk uint8
        [pair_cap] or None, status int32 [B]: GUIDE_OK / GUIDE_DEFERRED)"""
        fn, who, lead = self._rows_call("vigo_guide_assign", _n_pts, ctrl)
        B, N = ctrl.shape[0], ctrl.shape[1]
        d = self.device
        f = 0 if fill is None else int(fill)
        off = torch.full((B * N + 1,), f, dtype=torch.int32, device=d)
        pv = torch.full((max(int(pair_cap), 1), 6), float(f), dtype=torch.float64, device=d)
        unk = torch.full((max(int(pair_cap), 1),), f & 0xFF, dtype=torch.uint8, device=d) if want_unknown else None
        status = torch.full((max(B, 1),), -1 if fill is None else f, dtype=torch.int32, device=d)
        self._check(fn(
            *lead, _ptr(ctrl, torch.float64, "ctrl", d), _ptr(seg_off, torch.int32, "seg_off", d), _ptr(seg, torch.int32, "seg", d),
            _ptr(path_off, torch.int32, "path_off", d), _ptr(path, torch.float64, "path", d), int(pair_cap), C.c_void_p(off.data_ptr()),
            C.c_void_p(pv.data_ptr()), C.c_void_p(unk.data_ptr()) if want_unknown else None, C.c_void_p(status.data_ptr())),
            who)
        return off, pv[:int(pair_cap)], (unk[:int(pair_cap)] if want_unknown else None), status[:B]

    def guide_assign_mixed(self, n_pts, ctrl, seg_off, seg, path_off, path, pair_cap, want_unknown=True, fill=None):
        """vigo_guide_assign_mixed: guide_assign on rows of Ns control points (ctrl f64 [B,Ns,3]) of which n_pts[b] (int32 [B],
        device) are trajectory b's; guide_off is int32 [B*Ns+1], the padding's ranges empty: optimize_mixed takes it as it is"""
        return self.guide_assign(ctrl, seg_off, seg, path_off, path, pair_cap, want_unknown, fill, _n_pts=n_pts)

    def collision_segs(self, ctrl, not_check_ratio=0.0, seg_cap=None, fill=None, _n_pts=None):
        """vigo_collision_segs: findCollisionSeg for B trajectories (ctrl f64 [B,N,3]) -> (seg_off int32 [B+1], seg int32
        [seg_cap,2], status int32 [B]: PATHS_OK / PATHS_DEFERRED); seg_cap defaults to B * 48"""
        fn, who, lead = self._rows_call("vigo_collision_segs", _n_pts, ctrl)
        B = ctrl.shape[0]
        cap = B * 48 if seg_cap is None else int(seg_cap)
        d = self.device
        f = 0 if fill is None else int(fill)
        seg_off = torch.full((B + 1,), f, dtype=torch.int32, device=d)
        seg = torch.full((max(cap, 1), 2), f, dtype=torch.int32, device=d)
        status = torch.full((max(B, 1),), -1 if fill is None else f, dtype=torch.int32, device=d)
        self._check(fn(*lead, _ptr(ctrl, torch.float64, "ctrl", d), float(not_check_ratio), C.c_void_p(seg_off.data_ptr()),
                       C.c_void_p(seg.data_ptr()), cap, C.c_void_p(status.data_ptr())), who)
        return seg_off, seg[:cap], status[:B]

    def collision_segs_mixed(self, n_pts, ctrl, not_check_ratio=0.0, seg_cap=None, fill=None):
        """vigo_collision_segs_mixed: collision_segs on rows of Ns control points (ctrl f64 [B,Ns,3]) of which n_pts[b] (int32
        [B], device) are trajectory b's; a count outside [7, Ns] reads PATHS_DEFERRED"""
        return self.collision_segs(ctrl, not_check_ratio, seg_cap, fill, _n_pts=n_pts)

    def path_search(self, ctrl, step, pool, min_height, max_height, seg_off=None, seg=None, not_check_ratio=0.0, max_expansions=1 << 20,
                    search_path_cap=256, seg_cap=None, point_cap=None, want_counts=True, fill=None, _n_pts=None):
        """vigo_path_search: pathSearch for B trajectories (ctrl f64 [B,N,3]) on the scanned segments, or on a supplied list
        (seg_off int32 [B+1], seg int32 [S,2]) -> (status int32 [B]: PATHS_OK / PATHS_FAILED / PATHS_DEFERRED, seg_off int32
        [B+1], seg int32 [seg_cap,2], path_off int32 [seg_cap+1], path f64 [point_cap,3], counts int32 [B,2] or None): the
        seg_off / seg / path_off / path of guide_assign.  seg_cap defaults to B * 48, point_cap to seg_cap * (search_path_cap + 1)"""
        fn, who, lead = self._rows_call("vigo_path_search", _n_pts, ctrl)
        B = ctrl.shape[0]
        scap = B * 48 if seg_cap is None else int(seg_cap)
        pcap = min(scap * (int(search_path_cap) + 1), 1 << 24) if point_cap is None else int(point_cap)
        d = self.device
        f = 0 if fill is None else int(fill)
        status = torch.full((max(B, 1),), -1 if fill is None else f, dtype=torch.int32, device=d)
        o_seg_off = torch.full((B + 1,), f, dtype=torch.int32, device=d)
        o_seg = torch.full((max(scap, 1), 2), f, dtype=torch.int32, device=d)
        o_path_off = torch.full((max(scap, 0) + 1,), f, dtype=torch.int32, device=d)
        o_path = torch.full((max(pcap, 1), 3), float(f), dtype=torch.float64, device=d)
        counts = torch.full((max(B, 1), 2), f, dtype=torch.int32, device=d) if want_counts else None
        self._check(fn(
            *lead, _ptr(ctrl, torch.float64, "ctrl", d), None if seg_off is None else _ptr(seg_off, torch.int32, "seg_off", d),
            None if seg is None else _ptr(seg, torch.int32, "seg", d), float(not_check_ratio), float(step),
            (C.c_int32 * 3)(*[int(v) for v in pool]), float(min_height), float(max_height), int(max_expansions), int(search_path_cap), scap, pcap,
            C.c_void_p(status.data_ptr()), C.c_void_p(o_seg_off.data_ptr()), C.c_void_p(o_seg.data_ptr()), C.c_void_p(o_path_off.data_ptr()),
            C.c_void_p(o_path.data_ptr()), C.c_void_p(counts.data_ptr()) if want_counts else None), who)
        return status[:B], o_seg_off, o_seg[:scap], o_path_off, o_path[:pcap], (counts[:B] if want_counts else None)

    def path_search_mixed(self, n_pts, ctrl, step, pool, min_height, max_height, seg_off=None, seg=None, not_check_ratio=0.0,
                          max_expansions=1 << 20, search_path_cap=256, seg_cap=None, point_cap=None, want_counts=True, fill=None):
        """vigo_path_search_mixed: path_search on rows of Ns control points (ctrl f64 [B,Ns,3]) of which n_pts[b] (int32 [B],
        device) are trajectory b's; its outputs are the seg_off / seg / path_off / path of guide_assign_mixed"""
        return self.path_search(ctrl, step, pool, min_height, max_height, seg_off, seg, not_check_ratio, max_expansions, search_path_cap,
                                seg_cap, point_cap, want_counts, fill, _n_pts=n_pts)

    def rebound_reguide(self, ctrl, guide_off, guide_pv, guide_unk, weights, state, step, pool, min_height, max_height, pair_cap,
                        not_check_ratio=0.0, max_expansions=1 << 20, search_path_cap=256, seg_cap=None, point_cap=None, want_paths=True,
                        want_unknown=True, fill=0, _n_pts=None):
        """vigo_rebound_reguide: the re-guide step of the rebound loop for the NEEDS_HOST trajectories of a batch (ctrl f64
        [B,N,3]; the current guide CSR guide_off int32 [B*N+1] / guide_pv f64 [G,6] / guide_unk uint8 [G], or None: no guides).
        weights [B,4] and state [B, REBOUND_STATE_INTS] (int32) are updated in place.  -> (status int32 [B]: REGUIDE_*, the
        merged CSR off int32 [B*N+1], pv f64 [pair_cap,6], unk uint8 [pair_cap] or None, and the paths path_seg_off int32
        [B+1], path_off int32 [seg_cap+1], path f64 [point_cap,3] or three None).  seg_cap defaults to B * 48, point_cap to
        seg_cap * (search_path_cap + 1); the output buffers are pre-filled with `fill`."""
        fn, who, lead = self._rows_call("vigo_rebound_reguide", _n_pts, ctrl)
        B, N = ctrl.shape[0], ctrl.shape[1]
        _shape(state, (B, self.REBOUND_STATE_INTS), "state")
        _shape(weights, (B, 4), "weights")
        scap = B * 48 if seg_cap is None else int(seg_cap)
        pcap = min(scap * (int(search_path_cap) + 1), 1 << 24) if point_cap is None else int(point_cap)
        cap = int(pair_cap)
        d = self.device
        status = torch.full((max(B, 1),), fill, dtype=torch.int32, device=d)
        o_off = torch.full((B * N + 1,), fill, dtype=torch.int32, device=d)
        o_pv = torch.full((max(cap, 1), 6), float(fill), dtype=torch.float64, device=d)
        o_unk = torch.full((max(cap, 1),), fill & 0xFF, dtype=torch.uint8, device=d) if want_unknown else None
        p_so = torch.full((B + 1,), fill, dtype=torch.int32, device=d) if want_paths else None
        p_po = torch.full((max(scap, 0) + 1,), fill, dtype=torch.int32, device=d) if want_paths else None
        p_pa = torch.full((max(pcap, 1), 3), float(fill), dtype=torch.float64, device=d) if want_paths else None
        opt = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(fn(
            *lead, _ptr(ctrl, torch.float64, "ctrl", d), None if guide_off is None else _ptr(guide_off, torch.int32, "guide_off", d),
            None if guide_pv is None else _ptr(guide_pv, torch.float64, "guide_pv", d),
            None if guide_unk is None else _ptr(guide_unk, torch.uint8, "guide_unk", d), _ptr(weights, torch.float64, "weights", d),
            float(not_check_ratio), float(step), (C.c_int32 * 3)(*[int(v) for v in pool]), float(min_height), float(max_height), int(max_expansions),
            int(search_path_cap), _ptr(state, torch.int32, "state", d), cap, opt(o_off), opt(o_pv), opt(o_unk), scap, pcap, opt(p_so), opt(p_po),
            opt(p_pa), opt(status)), who)
        return status[:B], o_off, o_pv[:cap], (o_unk[:cap] if want_unknown else None), p_so, p_po, (p_pa[:pcap] if want_paths else None)

    def rebound_reguide_mixed(self, n_pts, ctrl, guide_off, guide_pv, guide_unk, weights, state, step, pool, min_height, max_height,
                              pair_cap, not_check_ratio=0.0, max_expansions=1 << 20, search_path_cap=256, seg_cap=None, point_cap=None,
                              want_paths=True, want_unknown=True, fill=0):
        """vigo_rebound_reguide_mixed: rebound_reguide on rows of Ns control points (ctrl f64 [B,Ns,3]) of which n_pts[b] (int32
        [B], device) are trajectory b's; both guide CSRs are int32 [B*Ns+1], as rebound_rounds_mixed takes them"""
        return self.rebound_reguide(ctrl, guide_off, guide_pv, guide_unk, weights, state, step, pool, min_height, max_height, pair_cap,
                                    not_check_ratio, max_expansions, search_path_cap, seg_cap, point_cap, want_paths, want_unknown, fill,
                                    _n_pts=n_pts)

    def poly_sample(self, coeffs, n_samp, delT, stride, want_f64=True, want_f32=False):
        """vigo_poly_sample: positions of polyTrajSolver::getTrajectory for S segments ->
        (pos f64 [S,stride,3] or None, pos f32 [S,stride,3] or None); rows k >= n_samp[s] are left untouched (zero)."""
        _shape(coeffs, (None, 3, None), "coeffs")
        S, _, d1 = coeffs.shape
        _shape(n_samp, (S,), "n_samp")
        _shape(delT, (S,), "delT")
        p64 = torch.zeros(S, stride, 3, dtype=torch.float64, device=self.device) if want_f64 else None
        p32 = torch.zeros(S, stride, 3, dtype=torch.float32, device=self.device) if want_f32 else None
        self._check(self._lib.vigo_poly_sample(
            self._h, S, d1 - 1, _ptr(coeffs, torch.float64, "coeffs", self.device),
            _ptr(n_samp, torch.int32, "n_samp", self.device), _ptr(delT, torch.float64, "delT", self.device), int(stride),
            C.c_void_p(p64.data_ptr()) if want_f64 else None, C.c_void_p(p32.data_ptr()) if want_f32 else None), "vigo_poly_sample")
        return p64, p32

    def box_collision_points(self, pts, box, map_res):
        """vigo_box_collision_points: pts [M,3] f64 -> uint8 [M]"""
        _shape(pts, (None, 3), "pts")
        M = pts.shape[0]
        out = torch.empty(M, dtype=torch.uint8, device=self.device)
        self._check(self._lib.vigo_box_collision_points(self._h, M, _ptr(pts, torch.float64, "pts", self.device),
                                                        (C.c_double * 3)(*box), float(map_res),
                                                        C.c_void_p(out.data_ptr())), "vigo_box_collision_points")
        return out

    # ---- ESDF ---------------------------------------------------------------------------
    def set_esdf(self, dist: torch.Tensor, origin, res: float):
        nx, ny, nz = dist.shape
        self._check(self._lib.vigo_set_esdf(self._h, nx, ny, nz, (C.c_double * 3)(*origin), float(res),
                                            _ptr(dist, torch.float32, "dist", self.device)), "vigo_set_esdf")

    def build_esdf(self, plane: int = 2, unknown_is_site: bool = False, return_lattice: bool = False, tracked: bool = False):
        """vigo_build_esdf: the signed Euclidean distance field of the current snapshot (sites: plane 2 = occupied or
        0 = inflated-occupied, with the unknown voxels when unknown_is_site), built on the device and installed as the
        handle's ESDF.  return_lattice: also the row-major float32 [nx,ny,nz] lattice.  tracked: vigo_build_esdf_tracked —
        the same field, and the handle keeps what update_esdf needs (12 bytes per voxel) and collects the boxes of
        update_grid_region / update_grid_region_host from now on."""
        lattice = None
        if return_lattice:
            if self._grid_meta is None:
                raise VigoError("build_esdf(return_lattice=True) before set_grid")
            lattice = torch.empty(self._grid_meta[:3], dtype=torch.float32, device=self.device)
        fn, name = (self._lib.vigo_build_esdf_tracked, "vigo_build_esdf_tracked") if tracked else (self._lib.vigo_build_esdf, "vigo_build_esdf")
        self._check(fn(self._h, int(plane), 1 if unknown_is_site else 0, None if lattice is None else C.c_void_p(lattice.data_ptr())), name)
        return lattice

    def update_esdf(self, return_lattice: bool = False, stats: bool = False):
        """vigo_update_esdf: after build_esdf(tracked=True), the installed field brought up to the snapshot as the region
        updates since the last call left it — bit for bit what a rebuild gives — stream-ordered.  return_lattice: the whole
        row-major float32 [nx,ny,nz] lattice; stats: a dict of box_lo, box_n (the pending box worked on), y_lines, x_lines
        (synchronises the stream).  Returns None, the lattice, the dict, or (lattice, dict)."""
        lattice = None
        if return_lattice:
            if self._grid_meta is None:
                raise VigoError("update_esdf(return_lattice=True) before set_grid")
            lattice = torch.empty(self._grid_meta[:3], dtype=torch.float32, device=self.device)
        st = _lib.VigoEsdfUpdateStats() if stats else None
        self._check(self._lib.vigo_update_esdf(self._h, None if lattice is None else C.c_void_p(lattice.data_ptr()),
                                               None if st is None else C.byref(st)), "vigo_update_esdf")
        if stats:
            return (lattice, st.as_dict()) if return_lattice else st.as_dict()
        return lattice

    def esdf_query(self, pts: torch.Tensor):
        _shape(pts, (None, 3), "pts")
        q = pts.shape[0]
        d = torch.empty(q, dtype=torch.float64, device=self.device)
        g = torch.empty(q, 3, dtype=torch.float64, device=self.device)
        self._check(self._lib.vigo_esdf_query(self._h, q, _ptr(pts, torch.float64, "pts", self.device),
                                              C.c_void_p(d.data_ptr()), C.c_void_p(g.data_ptr())), "vigo_esdf_query")
        return d, g

    def esdf_query_f32(self, pts: torch.Tensor, out: Optional[torch.Tensor] = None):
        """vigo_esdf_query_f32: pts float32 [Q,3] -> float32 [Q,4] = (distance, gradient)"""
        _shape(pts, (None, 3), "pts")
        q = pts.shape[0]
        if out is None:
            out = torch.empty(q, 4, dtype=torch.float32, device=self.device)
        _shape(out, (q, 4), "out")
        self._check(self._lib.vigo_esdf_query_f32(self._h, q, _ptr(pts, torch.float32, "pts", self.device),
                                                  _ptr(out, torch.float32, "out", self.device)), "vigo_esdf_query_f32")
        return out

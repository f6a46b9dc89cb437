"""Handle on the HIP context: one ``mind_ctx`` per (process, thread).

A planner uses the runtime of the thread that built it.  One thread per scene, each under its own
``torch.cuda.stream``, gives independent contexts/streams whose kernels overlap on the device (BASELINE config 3:
several scenes planned concurrently on one MI355X); the common single-threaded case sees one runtime per process."""
import os
import threading

_local = threading.local()


def get_runtime(device=None):
    """This thread's ``HipPredictor`` (predictor + tree-iLQR entry points), bound to the thread's current torch
    stream when first requested.  Raises without a GPU / library: the product path has no CPU fallback."""
    rt = getattr(_local, "rt", None)
    if rt is None:
        from .predictor import HipPredictor
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        rt = _local.rt = HipPredictor(device)
    elif device is not None and int(device) != rt.device.index:
        # one context per thread: a second device in the same thread would silently run on the first one
        raise RuntimeError(f"this thread's HIP runtime is bound to cuda:{rt.device.index}, cuda:{int(device)} was requested; "
                           "use one host thread (or process) per device, or reset_runtime() first")
    return rt


def new_runtime(device=None):
    """A further ``HipPredictor`` of this thread: its own ``mind_ctx`` on its own (new) torch stream.  For a driver that plans several
    scenes from ONE thread and wants their kernels to overlap on the device (bench.py --concurrent P --pipelined: scene i's contingency
    solves run while scene i + 1's AIME rounds do); the caller owns it (``close()``)."""
    import torch
    from .predictor import HipPredictor
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", int(device))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        rt = HipPredictor(int(device))
    rt.torch_stream = stream            # kept alive with the runtime; work the caller does through torch for this scene belongs on it
    return rt


def ilqr_gains(cfg, flats, x0, lane, target_vel, use_exo, us, mu, grid=None):
    """``HipPredictor.ilqr_gains`` on this thread's runtime: the gains of one backward pass about ``us`` on every cost tree."""
    return get_runtime().ilqr_gains(cfg, flats, x0, lane, target_vel, use_exo, us, mu, grid=grid)


def ilqr_policy_rollouts(cfg, flats, x0, lane, target_vel, use_exo, us, k, K, alpha, dx0=None, grid=None, want_xs=True, want_us=True,
                         want_L=True):
    """``HipPredictor.ilqr_policy_rollouts`` on this thread's runtime: closed-loop rollouts under the gains (k, K) about ``us``."""
    return get_runtime().ilqr_policy_rollouts(cfg, flats, x0, lane, target_vel, use_exo, us, k, K, alpha, dx0=dx0, grid=grid, want_xs=want_xs,
                                              want_us=want_us, want_L=want_L)


def audit_plan(flats, xs, ego_box, exo_margin):
    """``HipPredictor.audit_plan`` on this thread's runtime: clearance of candidate state sets on the cost trees of a plan."""
    return get_runtime().audit_plan(flats, xs, ego_box, exo_margin)


def audit_episode(ego_states, exo, valid, boxes, ego_box):
    """``HipPredictor.audit_episode`` on this thread's runtime: clearance of ego traces against one replayed scene."""
    return get_runtime().audit_episode(ego_states, exo, valid, boxes, ego_box)


def audit_ttc(ego_states, exo, valid, boxes, ego_box, horizon=3.0, bound=0.95, lanes=0):
    """``HipPredictor.audit_ttc`` on this thread's runtime: time to collision of ego traces against one replayed scene."""
    return get_runtime().audit_ttc(ego_states, exo, valid, boxes, ego_box, horizon, bound, lanes)


def audit_lane_plan(flats, xs, verts, lane_off, ego_box, cos_flow, bound, form=0):
    """``HipPredictor.audit_lane_plan`` on this thread's runtime: lane offset, heading and progress of candidate state sets on the cost trees
    of a plan."""
    return get_runtime().audit_lane_plan(flats, xs, verts, lane_off, ego_box, cos_flow, bound, form)


def audit_lane_episode(ego_states, verts, lane_off, ego_box, cos_flow, bound, form=0):
    """``HipPredictor.audit_lane_episode`` on this thread's runtime: lane offset, heading and progress of ego traces."""
    return get_runtime().audit_lane_episode(ego_states, verts, lane_off, ego_box, cos_flow, bound, form)


def audit_road_plan(flats, xs, verts, poly_off, ego_box):
    """``HipPredictor.audit_road_plan`` on this thread's runtime: road margin of candidate state sets on the cost trees of a plan."""
    return get_runtime().audit_road_plan(flats, xs, verts, poly_off, ego_box)


def audit_road_episode(ego_states, verts, poly_off, ego_box):
    """``HipPredictor.audit_road_episode`` on this thread's runtime: road margin of ego traces against a drivable area."""
    return get_runtime().audit_road_episode(ego_states, verts, poly_off, ego_box)


def forecast_score(reg, cls, actor_off, gt, valid, scored=None, **cfg):
    """``HipPredictor.forecast_score`` on this thread's runtime: a forecast on the device against recorded futures."""
    return get_runtime().forecast_score(reg, cls, actor_off, gt, valid, scored, **cfg)


def set_decoder_basis(name):
    """``HipPredictor.set_decoder_basis`` on this thread's runtime: 'bezier' | 'monomial' for every net and planner that shares it."""
    return get_runtime().set_decoder_basis(name)


def get_decoder_basis():
    """``HipPredictor.get_decoder_basis`` on this thread's runtime."""
    return get_runtime().get_decoder_basis()


def curve_eval(param, tau, basis=None, want=("reg", "vel", "cov_vel")):
    """``HipPredictor.curve_eval`` on this thread's runtime: the decoder's curves at the times ``tau`` from control points ``param``."""
    return get_runtime().curve_eval(param, tau, basis=basis, want=want)


def reset_runtime():
    rt = getattr(_local, "rt", None)
    if rt is not None:
        rt.close()
    _local.rt = None

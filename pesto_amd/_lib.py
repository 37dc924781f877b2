"""ctypes binding of libpesto_hip.so (the C ABI declared in include/pesto_hip.h), and where a call's arrays live (Side).

The library is built in-tree by ``python -m pesto_amd.csrc.build`` (hipcc --offload-arch=gfx950) and
must be present: there is NO fallback path - a missing library raises at first use.
"""
import ctypes
import os

import numpy as np

from .config import MAX_LAYERS, normalise

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PESTO_LIB") or os.path.join(_HERE, "csrc", "libpesto_hip.so")   # PESTO_LIB: developer builds

PTR_HOST, PTR_DEVICE = 0, 1
IDS_INT32, IDS_INT64, IDS_UINT16 = 32, 64, 16
IDS_NARROW = 0x100      # OR-ed to IDS_INT32 / IDS_INT64 (pesto_forward_batch_submit): staged as uint16, narrowed and range-checked by the packer
BATCH_COLLATED, BATCH_INDEPENDENT = 0, 1
# enum pesto_precision
PRECISIONS = {"auto": 0, "f16_split": 1, "fp32": 2}
ERR_RANGE = -5


class PestoConfig(ctypes.Structure):
    """struct pesto_config (include/pesto_hip.h)."""
    _fields_ = [
        ("n0", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("nn", ctypes.c_int32 * MAX_LAYERS),
        ("n_out", ctypes.c_int32),
        ("em_depth", ctypes.c_int32),
        ("dm_depth", ctypes.c_int32),
        ("precision", ctypes.c_int32),
    ]


def precision_code(precision):
    try:
        return PRECISIONS[str(precision).lower()]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}") from None


def make_c_config(config, precision="auto"):
    c = normalise(config)
    cc = PestoConfig()
    cc.n0 = c["em"]["N0"]
    cc.n_layers = len(c["sum"])
    for i, l in enumerate(c["sum"]):
        cc.nn[i] = l["nn"]
    cc.n_out = c["dm"]["N2"]
    cc.em_depth = c["em_depth"]
    cc.dm_depth = c["dm_depth"]
    cc.precision = precision_code(precision)
    return cc


# every symbol include/pesto_hip.h declares (tests/test_abi.py checks the built library exports them all)
ABI_SYMBOLS = [
    "pesto_last_error", "pesto_blob_size", "pesto_create", "pesto_destroy", "pesto_forward",
    "pesto_workspace_bytes", "pesto_synchronize", "pesto_set_timing", "pesto_get_timing",
    "pesto_stage_embed", "pesto_stage_unpack", "pesto_stage_layer", "pesto_stage_pool", "pesto_knn_collate",
    "pesto_forward_frames", "pesto_postprocess", "pesto_forward_batch", "pesto_get_kernel_timing",
    "pesto_set_precision", "pesto_get_status", "pesto_debug_select", "pesto_forward_structures",
    "pesto_mask_to_segments", "pesto_debug_edge_mode", "pesto_forward_batch_submit", "pesto_forward_batch_wait",
    "pesto_set_async_auto", "pesto_debug_host_only", "pesto_knn_tie_rows", "pesto_set_auto_state_limit", "pesto_set_auto_pad_trigger",
    "pesto_get_auto_counters", "pesto_interface_labels", "pesto_bc_scores", "pesto_eval_last_error",
    "pesto_interface_patches", "pesto_patches_last_error", "pesto_contacts", "pesto_contacts_last_error",
    "pesto_trajectory_last_error", "pesto_contact_counts", "pesto_contact_loglik", "pesto_contact_div_kl", "pesto_residue_contact_maps",
    "pesto_native_contacts", "pesto_superpose", "pesto_residue_centroids", "pesto_sasa_last_error", "pesto_sasa",
    "pesto_dssp_last_error", "pesto_dssp", "pesto_docking_last_error", "pesto_frame_contacts", "pesto_frame_residue_contacts",
    "pesto_interface_atoms", "pesto_rigid_docking", "pesto_interface_rmsd", "pesto_hbonds_last_error", "pesto_frame_hbonds",
    "pesto_hbond_occupancy", "pesto_unwrap_pbc",
    "pesto_cluster_last_error", "pesto_pairwise_rmsd", "pesto_gromos_clusters",
    "pesto_peaks_last_error", "pesto_weighted_centers", "pesto_pair_distance_rank", "pesto_density_peaks",
    "pesto_dockq_last_error", "pesto_dockq", "pesto_fit_rmsd",
    "pesto_poses_last_error", "pesto_poses_scores", "pesto_poses_slide", "pesto_poses_materialize", "pesto_poses_top",
    "pesto_lddt_last_error", "pesto_lddt_pairs", "pesto_lddt",
    "pesto_tmscore_last_error", "pesto_tmscore",
    "pesto_align_last_error", "pesto_align_scores", "pesto_align_maps",
    "pesto_structalign_last_error", "pesto_structalign",
    "pesto_chainmap_last_error", "pesto_chainmap",
    "pesto_qsscore_last_error", "pesto_qsscore", "pesto_qsmap",
    "pesto_dynamics_last_error", "pesto_fluctuations", "pesto_covariance", "pesto_cross_correlation", "pesto_pca", "pesto_project",
    "pesto_enm_last_error", "pesto_enm_network", "pesto_enm_matrix", "pesto_enm_modes", "pesto_enm_fluctuations", "pesto_enm_overlap",
    "pesto_enm_deform",
    "pesto_rank_last_error", "pesto_rank_scores", "pesto_rank_curves", "pesto_rank_histogram",
    "pesto_surface_last_error", "pesto_surface_nearest", "pesto_surface_areas", "pesto_surface_residues", "pesto_surface_vertex_scores",
    "pesto_surface_scored",
    "pesto_train_last_error", "pesto_train_create", "pesto_train_destroy", "pesto_train_step", "pesto_train_adam", "pesto_train_get_state",
    "pesto_train_set_state", "pesto_train_set_timing", "pesto_train_get_timing", "pesto_train_stage_embed", "pesto_train_stage_layer",
    "pesto_train_stage_head", "pesto_train_set_weights", "pesto_train_forward", "pesto_train_backward",
]

_lib = None


class PestoError(RuntimeError):
    """code: the negative pesto_status the library returned (None when raised by the Python layer)."""
    code = None


def load():
    """Load libpesto_hip.so (once). Raises PestoError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PestoError(f"{LIB_PATH} not found: build it with `python -m pesto_amd.csrc.build` "
                         "(there is no CPU/PyTorch fallback for the forward pass)")
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64. If this
    # library pulled in /opt/rocm's copy first, torch would later load a second runtime and one of the two
    # would see no device. Importing torch first makes the dynamic loader resolve our DT_NEEDED
    # libamdhip64.so.7 to the copy torch already mapped (SONAME match).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = ctypes.POINTER
    lib.pesto_last_error.restype = ctypes.c_char_p
    lib.pesto_last_error.argtypes = []
    lib.pesto_blob_size.argtypes = [P(PestoConfig), P(i64)]
    lib.pesto_create.argtypes = [P(PestoConfig), c_p, i64, ctypes.c_int, P(c_p)]
    lib.pesto_destroy.argtypes = [c_p]
    lib.pesto_forward.argtypes = [c_p, i64, i64, i32, c_p, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_forward_structures.argtypes = [c_p, i64, i64, i32, i32, c_p, c_p, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_forward_frames.argtypes = [c_p, i64, i64, i32, i64, c_p, i64, i64, c_p, i32, c_p, c_p, c_p, i32, i32, c_p]
    lib.pesto_forward_batch.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_forward_batch_submit.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, c_p, c_p, i32, c_p, c_p, c_p, i32, P(i32)]
    lib.pesto_forward_batch_wait.argtypes = [c_p, i32]
    lib.pesto_set_precision.argtypes = [c_p, i32]
    lib.pesto_set_async_auto.argtypes = [c_p, i32]
    lib.pesto_set_auto_state_limit.argtypes = [c_p, ctypes.c_float]
    lib.pesto_set_auto_pad_trigger.argtypes = [c_p, i32]
    lib.pesto_debug_host_only.argtypes = [c_p, i32]
    lib.pesto_get_status.argtypes = [c_p, P(i32), P(i64), P(i64)]
    lib.pesto_get_auto_counters.argtypes = [c_p, P(i64), P(i64)]
    lib.pesto_debug_select.argtypes = [c_p, i32, i32]
    lib.pesto_debug_edge_mode.argtypes = [c_p, i32]
    lib.pesto_mask_to_segments.argtypes = [c_p, i64, i64, c_p, c_p, i32, c_p]
    lib.pesto_postprocess.argtypes = [c_p, i64, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_workspace_bytes.argtypes = [c_p, i64, i64, P(i64)]
    lib.pesto_synchronize.argtypes = [c_p]
    lib.pesto_set_timing.argtypes = [c_p, i32]
    lib.pesto_get_timing.argtypes = [c_p, P(ctypes.c_double), P(ctypes.c_double), P(i32)]
    lib.pesto_get_kernel_timing.argtypes = [c_p, P(ctypes.c_double), P(i32)]
    lib.pesto_knn_collate.argtypes = [c_p, i64, i32, c_p, c_p, i32, c_p, i32, i32, c_p]
    lib.pesto_knn_tie_rows.argtypes = [c_p, i64, i32, c_p, c_p, i32, c_p, i32, c_p, i32, c_p]
    lib.pesto_eval_last_error.restype = ctypes.c_char_p
    lib.pesto_eval_last_error.argtypes = []
    lib.pesto_interface_labels.argtypes = [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i64, ctypes.c_float, c_p, c_p, i32, c_p]
    lib.pesto_bc_scores.argtypes = [c_p, i32, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_patches_last_error.restype = ctypes.c_char_p
    lib.pesto_patches_last_error.argtypes = []
    lib.pesto_interface_patches.argtypes = [c_p, i32, c_p, i32, c_p, c_p, c_p, c_p, i32, c_p, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                            c_p, c_p, c_p, c_p, i32, i32, c_p]
    lib.pesto_contacts_last_error.restype = ctypes.c_char_p
    lib.pesto_contacts_last_error.argtypes = []
    lib.pesto_contacts.argtypes = [c_p, i64, i32, c_p, i32, c_p, c_p, c_p, c_p, i32, ctypes.c_float, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p,
                                   c_p, c_p, i32, c_p]
    lib.pesto_trajectory_last_error.restype = ctypes.c_char_p
    lib.pesto_trajectory_last_error.argtypes = []
    lib.pesto_contact_counts.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, c_p, c_p, c_p, i32, i32, c_p]
    lib.pesto_contact_loglik.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_contact_div_kl.argtypes = [c_p, i64, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_residue_contact_maps.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, i32, c_p, c_p, c_p, c_p, ctypes.c_float, ctypes.c_float,
                                               c_p, i32, c_p]
    lib.pesto_native_contacts.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_superpose.argtypes = [c_p, i64, i64, i64, i64, i64, c_p, c_p, c_p, c_p, ctypes.c_double, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_residue_centroids.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_sasa_last_error.restype = ctypes.c_char_p
    lib.pesto_sasa_last_error.argtypes = []
    lib.pesto_sasa.argtypes = [c_p, i64, i64, i32, c_p, c_p, c_p, i32, c_p, ctypes.c_double, c_p, c_p, i32, c_p, c_p, c_p, i32, c_p]
    lib.pesto_dssp_last_error.restype = ctypes.c_char_p
    lib.pesto_dssp_last_error.argtypes = []
    lib.pesto_dssp.argtypes = [c_p, i64, i64, c_p, ctypes.c_double, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_docking_last_error.restype = ctypes.c_char_p
    lib.pesto_docking_last_error.argtypes = []
    lib.pesto_frame_contacts.argtypes = [c_p, i64, i64, i64, c_p, c_p, ctypes.c_float, ctypes.c_float, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_frame_residue_contacts.argtypes = [c_p, i64, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, i32, i32, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_interface_atoms.argtypes = [c_p, i64, c_p, i64, c_p, i64, c_p, c_p, i32, ctypes.c_float, ctypes.c_float, c_p, i32, c_p]
    lib.pesto_rigid_docking.argtypes = [c_p, i64, i64, i64, c_p, c_p, i64, c_p, i64, c_p, c_p, c_p, i32, c_p]
    lib.pesto_interface_rmsd.argtypes = [c_p, i64, i64, i64, c_p, c_p, i64, c_p, ctypes.c_double, c_p, i32, c_p]
    lib.pesto_dockq_last_error.restype = ctypes.c_char_p
    lib.pesto_dockq_last_error.argtypes = []
    lib.pesto_dockq.argtypes = [c_p, i64, i64, c_p, c_p, i64, c_p, i64, c_p, i64, c_p, i64, c_p, i64, c_p, ctypes.c_float, ctypes.c_double, c_p, c_p, c_p,
                                c_p, c_p, c_p, i32, c_p]
    lib.pesto_fit_rmsd.argtypes = [c_p, i64, i64, i64, c_p, c_p, i64, c_p, i64, c_p, ctypes.c_double, c_p, i32, c_p]
    lib.pesto_poses_last_error.restype = ctypes.c_char_p
    lib.pesto_poses_last_error.argtypes = []
    lib.pesto_poses_scores.argtypes = [c_p, i64, i64, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_poses_slide.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, ctypes.c_float, ctypes.c_float, c_p, c_p, c_p, i32, c_p]
    lib.pesto_poses_materialize.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_poses_top.argtypes = [c_p, i64, i64, c_p, c_p, i32, c_p, P(i64), i32, c_p]
    lib.pesto_lddt_last_error.restype = ctypes.c_char_p
    lib.pesto_lddt_last_error.argtypes = []
    lib.pesto_lddt_pairs.argtypes = [c_p, i64, i32, c_p, c_p, c_p, c_p, c_p, i32, ctypes.c_float, ctypes.c_double, i64, c_p, c_p, c_p, P(i64), i32, c_p]
    lib.pesto_lddt.argtypes = [c_p, i64, i64, i32, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, i32, i32, c_p, ctypes.c_float, ctypes.c_double,
                               i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_tmscore_last_error.restype = ctypes.c_char_p
    lib.pesto_tmscore_last_error.argtypes = []
    lib.pesto_tmscore.argtypes = [c_p, i64, i64, i32, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, ctypes.c_double, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                  i32, c_p]
    lib.pesto_align_last_error.restype = ctypes.c_char_p
    lib.pesto_align_last_error.argtypes = []
    lib.pesto_align_scores.argtypes = [c_p, i32, c_p, c_p, i32, c_p, i32, i32, i32, i32, i64, c_p, c_p, c_p, c_p, c_p, c_p, i32, i32, i32, c_p, i32, c_p]
    lib.pesto_align_maps.argtypes = [c_p, i32, c_p, c_p, i32, c_p, i32, i32, i32, i32, i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_structalign_last_error.restype = ctypes.c_char_p
    lib.pesto_structalign_last_error.argtypes = []
    lib.pesto_structalign.argtypes = [c_p, i32, c_p, c_p, c_p, i64, c_p, c_p, c_p, ctypes.c_double, i32, i32, ctypes.c_double, c_p, c_p, c_p, c_p, c_p,
                                      c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_chainmap_last_error.restype = ctypes.c_char_p
    lib.pesto_chainmap_last_error.argtypes = []
    lib.pesto_chainmap.argtypes = [c_p, i64, i64, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double, i32, ctypes.c_double,
                                   c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_qsscore_last_error.restype = ctypes.c_char_p
    lib.pesto_qsscore_last_error.argtypes = []
    lib.pesto_qsscore.argtypes = [c_p, i64, i64, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i64, ctypes.c_double, ctypes.c_double,
                                  c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_qsmap.argtypes = [c_p, i64, i64, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double, c_p, c_p, c_p,
                                c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_dynamics_last_error.restype = ctypes.c_char_p
    lib.pesto_dynamics_last_error.argtypes = []
    lib.pesto_fluctuations.argtypes = [c_p, i64, i64, i64, c_p, c_p, ctypes.c_double, c_p, c_p, i32, c_p]
    lib.pesto_covariance.argtypes = [c_p, i64, i64, i64, c_p, c_p, ctypes.c_double, i32, c_p, i32, c_p]
    lib.pesto_cross_correlation.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, i32, c_p]
    lib.pesto_pca.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, ctypes.c_double, i32, ctypes.c_double, i32, c_p, c_p, c_p, c_p, c_p,
                              P(ctypes.c_double), P(i32), i32, c_p]
    lib.pesto_project.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, c_p, c_p, ctypes.c_double, c_p, i32, c_p]
    lib.pesto_enm_last_error.restype = ctypes.c_char_p
    lib.pesto_enm_last_error.argtypes = []
    lib.pesto_enm_network.argtypes = [c_p, i64, i64, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, i64, c_p, c_p, c_p, P(i64),
                                      P(ctypes.c_double), i32, c_p]
    lib.pesto_enm_matrix.argtypes = [c_p, i64, i64, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, i32, c_p, i32, c_p]
    lib.pesto_enm_modes.argtypes = [c_p, i64, i64, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, i32, i32, ctypes.c_double, i32,
                                    c_p, c_p, c_p, P(ctypes.c_double), P(i64), P(i32), i32, c_p]
    lib.pesto_enm_fluctuations.argtypes = [c_p, i64, i64, i32, c_p, c_p, ctypes.c_double, c_p, c_p, i32, c_p]
    lib.pesto_enm_overlap.argtypes = [c_p, i64, i64, i64, c_p, c_p, i32, c_p, i32, c_p]
    lib.pesto_enm_deform.argtypes = [c_p, i64, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_hbonds_last_error.restype = ctypes.c_char_p
    lib.pesto_hbonds_last_error.argtypes = []
    lib.pesto_frame_hbonds.argtypes = [c_p, i64, i64, i64, i64, c_p, c_p, c_p, c_p, ctypes.c_float, ctypes.c_float, ctypes.c_double, i64, c_p, c_p,
                                       c_p, c_p, i32, c_p]
    lib.pesto_hbond_occupancy.argtypes = [c_p, i64, i64, i64, i64, c_p, c_p, c_p, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                          i64, c_p, c_p, c_p, i32, c_p]
    lib.pesto_unwrap_pbc.argtypes = [c_p, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_cluster_last_error.restype = ctypes.c_char_p
    lib.pesto_cluster_last_error.argtypes = []
    lib.pesto_pairwise_rmsd.argtypes = [c_p, i64, i64, i64, i64, c_p, c_p, c_p, ctypes.c_double, c_p, i32, c_p]
    lib.pesto_gromos_clusters.argtypes = [c_p, i64, c_p, ctypes.c_float, c_p, c_p, c_p, P(i32), i32, c_p]
    lib.pesto_peaks_last_error.restype = ctypes.c_char_p
    lib.pesto_peaks_last_error.argtypes = []
    lib.pesto_weighted_centers.argtypes = [c_p, i64, i64, c_p, c_p, i32, ctypes.c_float, c_p, c_p, c_p, i32, c_p]
    lib.pesto_pair_distance_rank.argtypes = [c_p, i64, i32, c_p, c_p, i64, c_p, i64, P(ctypes.c_float), i32, c_p]
    lib.pesto_density_peaks.argtypes = [c_p, i64, i32, c_p, c_p, i64, c_p, ctypes.c_float, i32, i32, ctypes.c_double, ctypes.c_float,
                                        c_p, c_p, c_p, c_p, c_p, c_p, c_p, P(i32), i32, c_p]
    lib.pesto_rank_last_error.restype = ctypes.c_char_p
    lib.pesto_rank_last_error.argtypes = []
    lib.pesto_rank_scores.argtypes = [c_p, i32, c_p, i32, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_rank_curves.argtypes = [c_p, i32, c_p, i32, c_p, c_p, i32, i64, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_rank_histogram.argtypes = [c_p, i32, c_p, i32, c_p, c_p, i32, c_p, c_p, i32, c_p]
    lib.pesto_surface_last_error.restype = ctypes.c_char_p
    lib.pesto_surface_last_error.argtypes = []
    lib.pesto_surface_nearest.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, i32, c_p, c_p, i32, c_p]
    lib.pesto_surface_areas.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_surface_residues.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_surface_vertex_scores.argtypes = [c_p, i64, i64, c_p, c_p, c_p, i32, c_p]
    lib.pesto_surface_scored.argtypes = [c_p, i32, c_p, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_train_last_error.restype = ctypes.c_char_p
    lib.pesto_train_last_error.argtypes = []
    lib.pesto_train_create.argtypes = [P(PestoConfig), c_p, i64, ctypes.c_int, ctypes.c_float, ctypes.c_float, P(c_p)]
    lib.pesto_train_destroy.argtypes = [c_p]
    lib.pesto_train_step.argtypes = [c_p, i32, i64, i64, i32, i32, c_p, c_p, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_train_adam.argtypes = [c_p, c_p]
    lib.pesto_train_set_weights.argtypes = [c_p, c_p, i32, c_p]
    lib.pesto_train_forward.argtypes = [c_p, i32, i64, i64, i32, c_p, c_p, i32, c_p, c_p, c_p, P(i64), i32, c_p]
    lib.pesto_train_backward.argtypes = [c_p, i64, c_p, c_p, c_p, c_p, i32, c_p]
    lib.pesto_train_get_state.argtypes = [c_p, c_p, c_p, P(i64), P(ctypes.c_float)]
    lib.pesto_train_set_state.argtypes = [c_p, c_p, P(i64), P(ctypes.c_float)]
    lib.pesto_train_set_timing.argtypes = [c_p, i32]
    lib.pesto_train_get_timing.argtypes = [c_p, P(ctypes.c_double)]
    lib.pesto_train_stage_embed.argtypes = [c_p, i64, c_p, c_p, c_p]
    lib.pesto_train_stage_layer.argtypes = [c_p, i32, i64, i32, c_p, c_p, i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.pesto_train_stage_head.argtypes = [c_p, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.pesto_stage_embed.argtypes = [c_p, i64, c_p, c_p]
    lib.pesto_stage_unpack.argtypes = [c_p, i64, i32, c_p, c_p, i32, c_p, c_p]
    lib.pesto_stage_layer.argtypes = [c_p, i32, c_p, c_p]
    lib.pesto_stage_pool.argtypes = [c_p, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p]
    for name in ABI_SYMBOLS:
        if name not in ("pesto_last_error", "pesto_eval_last_error", "pesto_patches_last_error", "pesto_contacts_last_error",
                        "pesto_trajectory_last_error", "pesto_sasa_last_error", "pesto_dssp_last_error", "pesto_docking_last_error",
                        "pesto_hbonds_last_error", "pesto_cluster_last_error", "pesto_peaks_last_error", "pesto_rank_last_error", "pesto_surface_last_error",
                        "pesto_train_last_error", "pesto_dockq_last_error", "pesto_lddt_last_error", "pesto_tmscore_last_error",
                        "pesto_dynamics_last_error", "pesto_align_last_error", "pesto_structalign_last_error", "pesto_chainmap_last_error",
                        "pesto_qsscore_last_error", "pesto_enm_last_error", "pesto_poses_last_error"):
            getattr(lib, name).restype = ctypes.c_int
    _lib = lib
    return lib


def check(rc, last_error=None):
    """Raises PestoError (code = rc) unless rc == 0. ``last_error``: the function that holds the message. There are twenty-four channels:
    pesto_last_error (the default: the forward pass and everything else of pesto_api) and one per analysis group, pesto_eval_last_error,
    pesto_patches_last_error, pesto_contacts_last_error, pesto_trajectory_last_error, pesto_sasa_last_error, pesto_dssp_last_error, pesto_docking_last_error,
    pesto_hbonds_last_error, pesto_cluster_last_error, pesto_peaks_last_error, pesto_dockq_last_error, pesto_poses_last_error, pesto_lddt_last_error, pesto_tmscore_last_error, pesto_align_last_error, pesto_structalign_last_error, pesto_chainmap_last_error, pesto_qsscore_last_error, pesto_dynamics_last_error, pesto_enm_last_error, pesto_rank_last_error, pesto_surface_last_error and pesto_train_last_error."""
    if rc != 0:
        msg = (last_error or load().pesto_last_error)()
        err = PestoError(f"libpesto_hip error {rc}: {msg.decode() if msg else '?'}")
        err.code = rc
        raise err


# ------------------------------------------------------------------ host / device marshalling
def is_torch(x):
    return hasattr(x, "detach") and hasattr(x, "device")


def host(a):
    """``a`` as a numpy array (a torch tensor is detached and copied to the host first)."""
    return a.detach().cpu().numpy() if is_torch(a) else np.asarray(a)


def offsets(sizes):
    """int32 [len(sizes) + 1]: the exclusive prefix sum of ``sizes`` (the structure offsets the entry points take, always host memory)."""
    sizes = [int(v) for v in sizes]
    offs = np.zeros(len(sizes) + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    return offs


def ids_kind(ids):
    """IDS_INT64 / IDS_INT32 of a neighbour table that put() placed as (np.int64, np.int32)."""
    return IDS_INT64 if str(ids.dtype).endswith("int64") else IDS_INT32


def _torch_dtype(dtype):
    import torch
    return torch.int32 if dtype == np.uint32 else getattr(torch, dtype.name)      # (uint32 travels as the int32 of the same bits)


class Side:
    """The memory of ONE library call, decided by its lead array (X, X_frames, z, M or ps[0]). A ROCm lead puts the call on the device:
    device pointers, torch's current stream of the lead's GPU, which must be the handle's ``gpu`` (RuntimeError otherwise). Any other lead
    puts it on the host: host pointers, stream None; the library stages the arrays. Every array of the call goes through put() / cat() /
    empty(), so it lives on the call's side: with a ROCm lead a host array is copied to the device, never passed as a host pointer."""

    def __init__(self, lead, gpu):
        self.torch_lead = is_torch(lead)
        self.device, self.stream, self.kind = None, None, PTR_HOST
        if self.torch_lead and lead.is_cuda:
            import torch
            if lead.device.index != gpu:
                raise RuntimeError(f"inputs are on cuda:{lead.device.index} but the model is on cuda:{gpu} (use .to())")
            self.device, self.kind = lead.device, PTR_DEVICE
            self.stream = torch.cuda.current_stream(self.device).cuda_stream

    def _tensor(self, a, dtype):
        """a as a torch tensor of dtype on this side's GPU (not necessarily contiguous)"""
        import torch
        if not is_torch(a):
            a = np.asarray(a, dtype)
            a = torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if dtype == np.uint32 else a))
        return a.detach().to(device=self.device, dtype=_torch_dtype(dtype))

    def put(self, a, dtype, shape=None, name="array", strided=False):
        """``a`` (numpy, CPU / ROCm tensor, list) as a contiguous array of ``dtype`` on this side: a numpy array on the host, a tensor on
        the device (uint32 as the int32 of the same bits). ``a`` itself comes back when it is one already - no copy, no kernel.
        dtype: one numpy dtype, or a tuple of those the call takes (``a``'s own if it is one of them, else the first).
        shape: the shape the call needs (ValueError otherwise). strided: a view whose innermost axis is contiguous is kept as it is
        (read in place; element strides: strides())."""
        if isinstance(dtype, tuple):
            own = str(a.dtype if hasattr(a, "dtype") else np.asarray(a).dtype).replace("torch.", "")
            dtype = next((d for d in dtype if np.dtype(d).name == own), dtype[0])
        dtype = np.dtype(dtype)
        if self.device is None:
            out = host(a)
            if not (strided and out.dtype == dtype and out.ndim and out.strides[-1] == out.itemsize
                    and all(s % out.itemsize == 0 for s in out.strides)):
                out = np.ascontiguousarray(out, dtype=dtype)
        else:
            out = a
            if not (is_torch(a) and a.device == self.device and a.dtype == _torch_dtype(dtype)
                    and (a.stride(-1) == 1 if strided else a.is_contiguous())):
                out = self._tensor(a, dtype).contiguous()
        if shape is not None and tuple(out.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}, got {list(out.shape)}")
        return out

    def cat(self, arrays, dtype):
        """The arrays one after the other along axis 0, as put(): one contiguous array of ``dtype`` on this side."""
        dtype = np.dtype(dtype)
        if self.device is None:
            return np.ascontiguousarray(np.concatenate([host(a) for a in arrays]), dtype=dtype)
        import torch
        return torch.cat([self._tensor(a, dtype) for a in arrays]).contiguous()

    def empty(self, shape, dtype):
        """An uninitialised output array on this side."""
        if self.device is None:
            return np.empty(shape, dtype)
        import torch
        return torch.empty(shape, dtype=_torch_dtype(np.dtype(dtype)), device=self.device)

    def ptr(self, a):
        """The address the library reads / writes ``a`` at (None: NULL). Refuses, before any library call, an array of the other side:
        a device call takes tensors on its GPU only, a host call numpy arrays only."""
        if a is None:
            return None
        if self.device is None:
            if not isinstance(a, np.ndarray):
                raise RuntimeError(f"a host call takes numpy arrays, got {type(a).__name__}")
            return a.ctypes.data
        if not (is_torch(a) and a.device == self.device):
            where = a.device if is_torch(a) else type(a).__name__
            raise RuntimeError(f"a device call on {self.device} takes tensors on that GPU, got {where}")
        return a.data_ptr()

    def result(self, a):
        """An output as the lead's kind: a CPU tensor for a CPU-tensor lead, else ``a`` as it is."""
        if a is None or self.device is not None or not self.torch_lead:
            return a
        import torch
        return torch.from_numpy(a)


def strides(a):
    """Element strides of a numpy array or a torch tensor."""
    return tuple(a.stride()) if is_torch(a) else tuple(s // a.itemsize for s in a.strides)

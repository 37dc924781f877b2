"""pesto_amd: MI355X-native (gfx950) drop-in for PeSTo's geometric-transformer forward pass.

Only the hot path ``Model(config).forward(X, ids_topk, q, M)`` (reference model/model.py:32-52) lives
here: a Python host mirror of the reference Module API over a C-ABI HIP library. See DESIGN.md.
"""
from .config import CONFIGS, config_i_v3_0, config_i_v3_1, config_i_v4_0, config_i_v4_1, config_model  # noqa: F401

__all__ = ["Model", "evaluate", "interface_labels", "bc_scoring", "benchmark_assemblies", "patches", "interface_patches",
           "interface_patches_batch", "residue_ca", "save_patches", "trajectory", "StatisticalContactsModel", "contacts_distribution", "contact_counts",
           "div_KL", "interface_ensemble_comparison", "residue_contact_maps", "native_contacts", "fnat", "superpose_transform", "superpose", "rmsd",
           "residue_centroids", "docking", "contacts", "frame_contacts", "frame_residue_contacts", "interface_atoms", "irmsd", "interface_rigid_docking", "hbonds", "frame_hbonds", "baker_hubbard",
           "hydrogen_bonds", "unwrap_pbc", "atomic_masses", "hbond_tables", "ranking", "roc_curve", "precision_recall_curve", "confidence_histogram",
           "surface", "nearest_atoms", "vertex_areas", "residue_surface", "benchmark_surfaces", "read_ply", "write_ply",
           "clustering", "pairwise_rmsd", "gromos_clusters", "cluster_frames",
           "peaks", "interface_centers", "weighted_centers", "distance_quantile", "density_peaks", "cluster_interface_frames",
           "dockq", "lrmsd", "fit_rmsd", "native_pairs", "capri_class",
           "poses", "pose_scores", "slide_to_contact", "materialize", "top_poses", "rotation_set", "poses_about", "guided_dock", "PoseScores",
           "lddt", "ilddt", "lddt_ca", "reference_pairs", "structure_lddt",
           "tmscore", "tm_score", "gdt", "tm_ca", "structure_tmscore",
           "sequences", "align_scores", "align_maps", "cluster_sequences", "split_clusters", "structure_sequences",
           "structalign", "align_structures", "tm_matrix", "ca_traces", "structure_align",
           "chainmap", "chain_map", "apply_mapping", "structure_chainmap",
           "qsscore", "qs_score", "qs_map", "n_mappings", "mapping_of_index", "interface_points", "structure_qsscore",
           "dynamics", "fluctuations", "rmsf", "covariance", "cross_correlation", "pca", "project", "PCA",
           "normalmodes", "network", "hessian", "kirchhoff", "anm", "gnm", "Modes", "mode_fluctuations", "mode_correlation", "overlap",
           "cumulative_overlap", "deform", "sample_amplitudes", "mode_path", "structure_modes",
           "CONFIGS", "config_model", "config_i_v4_1", "config_i_v4_0", "config_i_v3_0", "config_i_v3_1"]


def __getattr__(name):  # lazy: importing the package must not need torch or the built library
    if name == "Model":
        from .model import Model
        return Model
    if name in ("evaluate", "interface_labels", "bc_scoring", "benchmark_assemblies"):
        import importlib
        ev = importlib.import_module(".evaluate", __name__)
        return ev if name == "evaluate" else getattr(ev, name)
    if name in ("patches", "interface_patches", "interface_patches_batch", "residue_ca", "save_patches"):
        import importlib
        pa = importlib.import_module(".patches", __name__)
        return pa if name == "patches" else getattr(pa, name)
    if name in ("trajectory", "StatisticalContactsModel", "contacts_distribution", "contact_counts", "div_KL", "interface_ensemble_comparison",
                "residue_contact_maps", "native_contacts", "fnat", "superpose_transform", "superpose", "rmsd", "residue_centroids"):
        import importlib
        tr = importlib.import_module(".trajectory", __name__)
        return tr if name == "trajectory" else getattr(tr, name)
    if name in ("docking", "contacts", "frame_contacts", "frame_residue_contacts", "interface_atoms", "irmsd", "interface_rigid_docking"):
        import importlib
        dk = importlib.import_module(".docking", __name__)
        return dk if name == "docking" else getattr(dk, name)
    if name in ("hbonds", "frame_hbonds", "baker_hubbard", "hydrogen_bonds", "unwrap_pbc", "atomic_masses", "hbond_tables"):
        import importlib
        hb = importlib.import_module(".hbonds", __name__)
        return hb if name == "hbonds" else getattr(hb, name)
    if name in ("ranking", "roc_curve", "precision_recall_curve", "confidence_histogram"):
        import importlib
        rk = importlib.import_module(".ranking", __name__)
        return rk if name == "ranking" else getattr(rk, name)
    if name in ("surface", "nearest_atoms", "vertex_areas", "residue_surface", "benchmark_surfaces", "read_ply", "write_ply"):
        import importlib
        sf = importlib.import_module(".surface", __name__)
        return sf if name == "surface" else getattr(sf, name)
    if name in ("clustering", "pairwise_rmsd", "gromos_clusters", "cluster_frames"):
        import importlib
        cl = importlib.import_module(".clustering", __name__)
        return cl if name == "clustering" else getattr(cl, name)
    if name in ("peaks", "interface_centers", "weighted_centers", "distance_quantile", "density_peaks", "cluster_interface_frames"):
        import importlib
        pk = importlib.import_module(".peaks", __name__)
        return pk if name == "peaks" else getattr(pk, name)
    if name in ("dockq", "lrmsd", "fit_rmsd", "native_pairs", "capri_class"):          # (dockq: the module; its function is dockq.dockq)
        import importlib
        dq = importlib.import_module(".dockq", __name__)
        return dq if name == "dockq" else getattr(dq, name)
    if name in ("poses", "pose_scores", "slide_to_contact", "materialize", "top_poses", "rotation_set", "poses_about", "guided_dock", "PoseScores"):
        import importlib
        ps = importlib.import_module(".poses", __name__)
        return ps if name == "poses" else getattr(ps, name)
    if name in ("lddt", "ilddt", "lddt_ca", "reference_pairs", "structure_lddt"):     # (lddt: the module; its function is lddt.lddt)
        import importlib
        ld = importlib.import_module(".lddt", __name__)
        return ld if name == "lddt" else getattr(ld, name)
    if name in ("tmscore", "tm_score", "gdt", "tm_ca", "structure_tmscore"):
        import importlib
        tm = importlib.import_module(".tmscore", __name__)
        return tm if name == "tmscore" else getattr(tm, name)
    if name in ("sequences", "align_scores", "align_maps", "cluster_sequences", "split_clusters", "structure_sequences"):
        import importlib
        sq = importlib.import_module(".sequences", __name__)
        return sq if name == "sequences" else getattr(sq, name)
    if name in ("structalign", "align_structures", "tm_matrix", "ca_traces", "structure_align"):
        import importlib
        sa = importlib.import_module(".structalign", __name__)
        return sa if name == "structalign" else getattr(sa, name)
    if name in ("chainmap", "chain_map", "apply_mapping", "structure_chainmap"):
        import importlib
        cm = importlib.import_module(".chainmap", __name__)
        return cm if name == "chainmap" else getattr(cm, name)
    if name in ("qsscore", "qs_score", "qs_map", "n_mappings", "mapping_of_index", "interface_points", "structure_qsscore"):
        import importlib
        qs = importlib.import_module(".qsscore", __name__)
        return qs if name == "qsscore" else getattr(qs, name)
    if name in ("dynamics", "fluctuations", "rmsf", "covariance", "cross_correlation", "pca", "project", "PCA"):
        import importlib
        dy = importlib.import_module(".dynamics", __name__)
        return dy if name == "dynamics" else getattr(dy, name)
    if name in ("normalmodes", "network", "hessian", "kirchhoff", "anm", "gnm", "Modes", "mode_fluctuations", "mode_correlation", "overlap",
                "cumulative_overlap", "deform", "sample_amplitudes", "mode_path", "structure_modes"):
        import importlib
        nm = importlib.import_module(".normalmodes", __name__)
        return nm if name == "normalmodes" else getattr(nm, name)
    raise AttributeError(name)

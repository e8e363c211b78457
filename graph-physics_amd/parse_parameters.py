"""JSON ``training_config`` surface for the MeshGraphNet path: same keys as the
reference factories (graphphysics/training/parse_parameters.py:81-190)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from .layers import set_use_silu_activation
from .losses import LossType, MultiLoss, PHYSICS_LOSSES, check_gradient_method
from .nodetype import NodeType
from .processors import EncodeProcessDecode
from .simulator import Simulator


def get_preprocessing(param: Dict[str, Any], device: torch.device, use_edge_feature: bool = True, remove_noise: bool = False,
                      extra_node_features=None, extra_edge_features=None, use_partitioning: bool = False,
                      num_partitions: Optional[int] = None, max_nodes_per_partition: Optional[int] = None,
                      masking_ratio: Optional[float] = None):
    """The preprocessing callable of a config (training/parse_parameters.py:24-78): reads
    ``transformations.preprocessing.noise`` / ``noise_index_start`` / ``noise_index_end``,
    ``transformations.world_pos_parameters`` and ``index.node_type_index`` and returns
    ``preprocess.build_preprocessing(...)``, a callable ``f(graph, step=0)`` over tensors on ``device`` (constructing it
    needs no GPU).

    The one place where the split differs from the reference: the reference honours ``dataset.khop`` in its Dataset class
    (training/parse_parameters.py:224, dataset/dataset.py:206-242); the engine has no Dataset class, so the key is read
    here and the k-hop expansion becomes the last step of the callable, with a per-trajectory cache keyed by
    ``graph.traj_index``.  ``dataset.khop`` defaults to 1; a non-integer or a value below 1 is a ``ValueError``.
    ``dataset.new_edges_ratio`` (random extra edges per sample, ``preprocess.add_random_edges``) is read here for the same
    reason: ``None`` or 0 is off; a value in ``(0, 1]`` is handed on as ``new_edges_ratio`` when ``device`` is a GPU (``cuda``);
    the sampler has no host path, so on any other device the key raises ``NotImplementedError`` when the callable is built
    rather than at the first sample.  A non-number, a bool or a value outside ``[0, 1]`` is a ``ValueError`` (the reference
    silently ignores a ratio above 1).  The reference freezes a frame's draw while the frame sits in its LRU frame cache; the
    engine has no Dataset class and draws per ``(seed, step)``.

    ``use_partitioning`` with ``num_partitions`` or ``max_nodes_per_partition`` are the reference's ``get_dataset`` arguments
    of the same names (train.py ``--use_partitioning --num_partitions / --max_nodes_per_partition``): every sample becomes one
    part of the mesh, cut as the last step (``preprocess.build_preprocessing(partitioning=...)``), and the callable takes a
    keyword ``part``.  Naming both counts or neither is the reference's ``ValueError``.  A part carries no ``face``: a config
    whose loss section needs it (physics terms with ``gradient_method: least_squares``) is refused here with a ``ValueError``,
    not by the first training step.  Without ``use_partitioning`` the two counts are ignored, as in the reference.

    ``masking_ratio`` is the reference's ``get_dataset(..., masking_ratio=...)`` argument: with a number in ``[0, 1]`` the callable
    returns ``(graph, selected_indices)`` (``preprocess.build_preprocessing(masking_ratio=...)``; the draw comes after k-hop and the
    random edges).  A bool, a non-number or a value outside ``[0, 1]`` is a ``ValueError``, and so is ``masking_ratio`` together with
    ``use_partitioning`` (the reference marks the combination "not working").  The reference freezes a frame's draw while the frame
    sits in its LRU frame cache; the engine draws per ``(seed, step)``.  ``None`` leaves the callable as it is."""
    from .preprocess import build_preprocessing

    prep = param.get("transformations", {}).get("preprocessing", {})
    noise_scale = prep.get("noise", 0)
    noise_parameters = None
    if noise_scale != 0 and not remove_noise:
        noise_parameters = {"noise_index_start": prep.get("noise_index_start"), "noise_index_end": prep.get("noise_index_end"),
                            "noise_scale": noise_scale, "node_type_index": param["index"]["node_type_index"]}
    world = param.get("transformations", {}).get("world_pos_parameters", {})
    world_pos_parameters = None
    if world.get("use", False):
        world_pos_parameters = {"world_pos_index_start": world.get("world_pos_index_start"),
                                "world_pos_index_end": world.get("world_pos_index_end"),
                                "node_type_index": param["index"]["node_type_index"]}
    dataset = param.get("dataset", {})
    khop = dataset.get("khop", 1)
    if isinstance(khop, bool) or not isinstance(khop, int) or khop < 1:
        raise ValueError(f"dataset.khop: an integer >= 1, got {khop!r}")
    ratio = dataset.get("new_edges_ratio", 0)
    if ratio is None:
        ratio = 0
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0 <= ratio <= 1:
        raise ValueError(f"dataset.new_edges_ratio: a number in [0, 1], got {ratio!r}")
    extra = {}
    if masking_ratio is not None:
        from .meshmask import check_masking_ratio

        extra["masking_ratio"] = check_masking_ratio(masking_ratio)
        if use_partitioning:
            raise ValueError("masking_ratio and use_partitioning cannot be combined (masking a partitioned sample is not supported, as "
                             "in the reference)")
    if ratio > 0:
        if torch.device(device).type != "cuda":
            raise NotImplementedError("dataset.new_edges_ratio: random extra edges are drawn by GPU kernels only (there is no host "
                                      f"path); got device {str(device)!r}")
        extra["new_edges_ratio"] = float(ratio)
    if use_partitioning:
        from .preprocess import num_partitions_for

        num_partitions_for(1, num_partitions, max_nodes_per_partition)   # both / neither: the reference's errors
        check_partitioned_loss(param)
        extra["partitioning"] = {"num_partitions": num_partitions, "max_nodes_per_partition": max_nodes_per_partition}
    return build_preprocessing(noise_parameters=noise_parameters, world_pos_parameters=world_pos_parameters,
                               add_edges_features=use_edge_feature, extra_node_features=extra_node_features,
                               extra_edge_features=extra_edge_features, khop=khop, khop_cache={} if khop > 1 else None, **extra)


def check_partitioned_loss(param: Dict[str, Any], loss=None) -> None:
    """``ValueError`` when the loss of the config (or ``loss``, a loss object, with the config's ``loss.gradient_method``)
    reads ``graph.face``: the parts of a partitioned mesh carry none (``preprocess.apply_partition``, as upstream)."""
    if loss is None:
        loss = get_loss(param)[0]
    if isinstance(loss, MultiLoss) and loss.needs_physical_fields and get_gradient_method(param) == "least_squares":
        raise ValueError("use_partitioning: the physics losses with gradient_method 'least_squares' need graph.face, which the parts "
                         "of a partitioned mesh do not carry (cut edges and faces are dropped); use 'finite_diff' or train unpartitioned")


def get_model(param: Dict[str, Any], only_processor: bool = False):
    model = param.get("model", {})
    model_type = model.get("type", "")
    node_input_size = param["model"]["node_input_size"] + NodeType.SIZE  # parse_parameters.py:96
    training = param.get("training", {})
    set_use_silu_activation(model.get("use_silu_activation", False))
    if model_type == "epd":
        return EncodeProcessDecode(
            message_passing_num=param["model"]["message_passing_num"],
            node_input_size=node_input_size,
            edge_input_size=param["model"]["edge_input_size"],
            output_size=param["model"]["output_size"],
            hidden_size=param["model"]["hidden_size"],
            only_processor=only_processor,
            use_rope_embeddings=model.get("use_rope_embeddings", False),
            use_gated_attention=model.get("use_gated_attention", False),
            use_gated_mlp=model.get("use_gated_mlp", False),
            rope_pos_dimension=model.get("rope_pos_dimension", 3),
            rope_base=model.get("rope_base", 10000.0),
            use_temporal_block=training.get("use_temporal_block", False),
        )
    if model_type == "transformer":  # parse_parameters.py:129-142
        from .transformer import EncodeTransformDecode
        return EncodeTransformDecode(
            message_passing_num=param["model"]["message_passing_num"],
            node_input_size=node_input_size,
            output_size=param["model"]["output_size"],
            hidden_size=param["model"]["hidden_size"],
            num_heads=param["model"]["num_heads"],
            only_processor=only_processor,
            use_rope_embeddings=model.get("use_rope_embeddings", False),
            use_gated_attention=model.get("use_gated_attention", False),
            rope_pos_dimension=model.get("rope_pos_dimension", 3),
            rope_base=model.get("rope_base", 10000.0),
            use_temporal_block=training.get("use_temporal_block", False),
        )
    if model_type == "transolver":
        raise NotImplementedError("model type 'transolver' is outside the message-passing hot path (SURVEY.md 7b)")
    raise ValueError(f"Model type '{model_type}' not supported.")


def get_transolver(param: Dict[str, Any]):
    """The ``TransolverProcessor`` of a ``model.type: "transolver"`` config, with the reference's keys and defaults
    (training/parse_parameters.py:95-160): ``message_passing_num``, ``hidden_size``, ``num_heads``, ``output_size``, ``dropout`` 0.0,
    ``mlp_ratio`` 1, ``slice_num`` 32, ``ref`` 8, ``unified_pos``, ``use_rope_embeddings``, ``rope_pos_dimension`` 3, ``rope_base`` 10000,
    ``use_gated_attention`` and ``training.use_temporal_block``.

    ``get_model`` deliberately STILL refuses this type with its ``NotImplementedError`` (a test pins that refusal, message included):
    the model is reached through this factory and through ``Engine``, which calls it for this type.  A later change flips
    ``get_model`` and that test together."""
    from .transolver import TransolverProcessor

    model = param.get("model", {})
    if model.get("type", "") != "transolver":
        raise ValueError(f"get_transolver: model.type is {model.get('type', '')!r}, not 'transolver'")
    training = param.get("training", {}) or {}
    return TransolverProcessor(
        message_passing_num=param["model"]["message_passing_num"],
        node_input_size=param["model"]["node_input_size"] + NodeType.SIZE,
        output_size=param["model"]["output_size"],
        hidden_size=param["model"]["hidden_size"],
        num_heads=param["model"]["num_heads"],
        dropout=model.get("dropout", 0.0),
        mlp_ratio=model.get("mlp_ratio", 1),
        slice_num=model.get("slice_num", 32),
        ref=model.get("ref", 8),
        unified_pos=model.get("unified_pos", False),
        use_rope_embeddings=model.get("use_rope_embeddings", False),
        use_gated_attention=model.get("use_gated_attention", False),
        rope_pos_dimension=model.get("rope_pos_dimension", 3),
        rope_base=model.get("rope_base", 10000.0),
        use_temporal_block=training.get("use_temporal_block", False),
    )


def get_simulator(param: Dict[str, Any], model, device: torch.device) -> Simulator:
    return Simulator(
        node_input_size=param["model"]["node_input_size"] + NodeType.SIZE,
        edge_input_size=param["model"]["edge_input_size"],
        output_size=param["model"]["output_size"],
        feature_index_start=param["index"]["feature_index_start"],
        feature_index_end=param["index"]["feature_index_end"],
        output_index_start=param["index"]["output_index_start"],
        output_index_end=param["index"]["output_index_end"],
        node_type_index=param["index"]["node_type_index"],
        model=model,
        device=device,
    )


def _loss_type(name: str) -> LossType:
    try:
        return LossType[str(name).upper()]
    except KeyError:
        raise ValueError(f"loss.type: unknown loss '{name}' (one of {', '.join(t.name.lower() for t in LossType)})") from None


def get_gradient_method(param: Dict[str, Any], **kwargs) -> Optional[str]:
    """``loss.gradient_method`` ("finite_diff" / "least_squares"), or None when the config names none
    (training/parse_parameters.py:326-340)"""
    try:
        method = param["loss"]["gradient_method"]
    except KeyError:
        return None
    return None if method is None else check_gradient_method(method)


def get_loss(param: Dict[str, Any], **kwargs) -> Tuple[Any, Union[str, List[str]]]:
    """The loss object of the config's ``loss`` section and its name(s) (training/parse_parameters.py:300-323): no section ->
    ``L2Loss``, one type -> that loss and its ``LossType`` name, several -> ``MultiLoss`` and the list of names.

    Configurations the reference accepts here and then fails on inside the first training step (a ``NameError`` /
    ``TypeError``) are refused now, with a ``ValueError`` that names the key."""
    if "loss" not in param:
        return LossType.L2LOSS.value(**kwargs), LossType.L2LOSS.name
    section = param["loss"]
    types = section.get("type")
    if isinstance(types, str) or not types:
        raise ValueError("loss.type: a non-empty list of loss names")
    kinds = [_loss_type(t) for t in types]
    method = get_gradient_method(param)   # validates the name
    if len(kinds) > 1:
        weights = section.get("weights")
        if weights is None or len(weights) != len(kinds):
            raise ValueError(f"loss.weights: {0 if weights is None else len(weights)} weights for {len(kinds)} loss types")
        if method is None:
            raise ValueError("loss.gradient_method: several loss types need a gradient method ('finite_diff' or 'least_squares')")
        return MultiLoss([k.value(**kwargs) for k in kinds], list(weights)), [k.name for k in kinds]
    if "weights" in section and section["weights"] is not None and len(section["weights"]) != 1:
        raise ValueError(f"loss.weights: {len(section['weights'])} weights for 1 loss type")
    if kinds[0] in PHYSICS_LOSSES:
        raise ValueError(f"loss.type: '{types[0]}' alone is not trainable: the single-loss training step passes no physical fields; "
                         "list it with at least one more loss type")
    return kinds[0].value(**kwargs), kinds[0].name


def matrix_precision_from_config(param: Dict[str, Any]) -> str:
    """``training.enable_vram_optimizations`` is the reference's switch to Lightning
    ``precision="bf16-mixed"`` (train.py:74-78,268-293): bf16 GEMM inputs, fp32 accumulate,
    fp32 RMSNorm / residual stream.  Here that is the engine's "bf16" matrix mode."""
    return "bf16" if param.get("training", {}).get("enable_vram_optimizations", False) else "fp32"


#: the spatial-MTP keys of the ``training`` section and their defaults (training/lightning_module.py:133-149)
SPATIAL_MTP_DEFAULTS = {"spatial_mtp_alpha": 0.20, "spatial_mtp_centers_per_step": 256, "spatial_mtp_num_heads": 4,
                        "spatial_mtp_num_layers": 1, "spatial_mtp_assume_undirected": True, "spatial_mtp_max_neighbors": None}


def get_spatial_mtp(param: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The spatial-MTP settings of the ``training`` section (``SPATIAL_MTP_DEFAULTS``), or None when ``training.use_spatial_mtp`` is
    false or absent.  Values the reference would fail on inside its first step, or that the HIP kernels do not cover, raise a
    ``ValueError`` that names the key."""
    training = param.get("training", {}) or {}
    if not training.get("use_spatial_mtp", False):
        return None
    out = {k: training.get(k, v) for k, v in SPATIAL_MTP_DEFAULTS.items()}
    for k in ("spatial_mtp_centers_per_step", "spatial_mtp_num_heads", "spatial_mtp_num_layers"):
        if isinstance(out[k], bool) or not isinstance(out[k], int) or out[k] < 1:
            raise ValueError(f"training.{k}: a positive integer, got {out[k]!r}")
    k = "spatial_mtp_max_neighbors"
    if out[k] is not None and (isinstance(out[k], bool) or not isinstance(out[k], int) or out[k] < 1):
        raise ValueError(f"training.{k}: None or a positive integer, got {out[k]!r}")
    hidden = param.get("model", {}).get("hidden_size")
    if hidden not in (16, 32, 64, 128):
        raise ValueError(f"model.hidden_size: training.use_spatial_mtp runs on the dense HIP kernels, which take 16, 32, 64 or 128 "
                         f"columns, got {hidden!r}")
    heads = out["spatial_mtp_num_heads"]
    if hidden % heads != 0 or heads not in (1, 2, 4, 8, 16):
        raise ValueError(f"training.spatial_mtp_num_heads: {heads} heads must divide model.hidden_size={hidden} and be one of 1, 2, 4, 8, 16")
    out["spatial_mtp_alpha"] = float(out["spatial_mtp_alpha"])
    out["spatial_mtp_assume_undirected"] = bool(out["spatial_mtp_assume_undirected"])
    return out


def cylinder_config(message_passing_num: int = 15, hidden_size: int = 128) -> Dict[str, Any]:
    """training_config/cylinder.json with the two benchmark overrides
    (message_passing_num 5->15, hidden_size 32->128; SURVEY.md TL;DR item 1)."""
    return {
        "model": {"type": "epd", "message_passing_num": message_passing_num, "hidden_size": hidden_size,
                  "node_input_size": 2, "output_size": 2, "edge_input_size": 3,
                  "use_silu_activation": False, "use_gated_mlp": False},
        "index": {"feature_index_start": 0, "feature_index_end": 2, "output_index_start": 0,
                  "output_index_end": 2, "node_type_index": 2},
        "training": {"use_spatial_mtp": False, "use_temporal_block": False, "enable_vram_optimizations": False},
    }


def plate_config(message_passing_num: int = 15, hidden_size: int = 128) -> Dict[str, Any]:
    """training_config/plate.json run through the message-passing engine (SURVEY.md TL;DR item 2: ``type: "epd"``,
    ``edge_input_size: 4`` = 3-D Cartesian + distance) under Lightning bf16-mixed (``enable_vram_optimizations``,
    train.py:74-78) -- BASELINE.json configs[2]."""
    return {
        "model": {"type": "epd", "message_passing_num": message_passing_num, "hidden_size": hidden_size,
                  "node_input_size": 6, "output_size": 3, "edge_input_size": 4},
        "index": {"feature_index_start": 0, "feature_index_end": 6, "output_index_start": 0, "output_index_end": 3,
                  "node_type_index": 6},
        "training": {"use_spatial_mtp": False, "use_temporal_block": False, "enable_vram_optimizations": True},
    }

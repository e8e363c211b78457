"""graph_physics_amd: MI355X-native MeshGraphNet message-passing engine behind the
Encoder/Processor/Decoder module API of DonsetPG/graph-physics."""
from .nodetype import NodeType  # noqa: F401
from .mesh import Graph, collate, cylinder_mesh, cylinder_batch, square_mesh, plate_mesh  # noqa: F401
from .layers import GraphNetBlock, Normalizer, RMSNorm, build_mlp  # noqa: F401
from .processors import EncodeProcessDecode  # noqa: F401
from .transformer import Attention, EncodeTransformDecode, TemporalAttention, Transformer  # noqa: F401
from .simulator import Simulator  # noqa: F401
from .parse_parameters import get_model, get_simulator, cylinder_config, plate_config, matrix_precision_from_config  # noqa: F401
from .parse_parameters import get_loss, get_gradient_method, get_preprocessing, get_spatial_mtp  # noqa: F401
from .spatial_mtp import SpatialMTP1Hop, star_attention  # noqa: F401
from .transolver import TransolverProcessor  # noqa: F401
from .parse_parameters import get_transolver  # noqa: F401
from .losses import (LossType, MultiLoss, L2Loss, CosineLoss, L1SmoothLoss, GradientL2Loss, ConvectionL2Loss, DivergenceL2Loss,  # noqa: F401
                     DivergenceL1Loss, DivergenceL1SmoothLoss, LossGeometry, compute_gradient)
from .ops import set_matrix_precision, get_matrix_precision, set_node_renumbering, get_node_renumbering  # noqa: F401
from . import preprocess  # noqa: F401
from . import meshmask  # noqa: F401
from .meshmask import get_masked_indexes, filter_edges, build_masked_graph, reconstruct_graph  # noqa: F401
from .preprocess import knn, knn_graph, min_distance_to_type  # noqa: F401
from .hierarchical_pooling import DownSampler, UpSampler, knn_interpolate  # noqa: F401

__version__ = "0.1.0"

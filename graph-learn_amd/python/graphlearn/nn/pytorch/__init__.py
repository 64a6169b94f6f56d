"""graphlearn.nn.pytorch (graphlearn/python/nn/pytorch): the torch side of graphlearn.nn."""
from graphlearn.nn.pytorch.data.dataset import Dataset  # noqa: F401
from graphlearn.nn.pytorch.segment import gather_rows, segment_aggregate, weighted_segment_aggregate  # noqa: F401

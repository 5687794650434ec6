"""numpy restatement of the dataframe-id lookup that the index conversion performs on the device
(sknnr_amd/csrc/narrow.hip.h, "indices, id table"; include/sknnr_hip.h, "Dataframe ids on the device").  Shared by
test_id_table_cpu.py, test_id_table_kernels_gpu.py and test_stream_ids_gpu.py."""

from __future__ import annotations

import numpy as np


def lookup(idx, table, fill=-1, dtype=np.int64):
    """``table[idx]`` where ``idx >= 0`` and ``fill`` elsewhere, as ``dtype``: the sign is tested on the index, and a
    negative index never reaches the table."""
    idx = np.asarray(idx)
    table = np.asarray(table)
    return np.where(idx < 0, fill, table[np.where(idx < 0, 0, idx)]).astype(dtype)

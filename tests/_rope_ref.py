"""The dense torch reference of the module with rotary position embedding: the rotation and the
module by its definition of ``tests/_module_ref.py``, under the names the rope tests import."""
from _module_ref import dense_attn, dense_run, rotate  # noqa: F401

"""lib/common/hand_skinning.py of the reference -> the HIP FK kernels (absolutetrack_amd.hand.skin_landmarks, and
skin_mesh: the reference's _skin_points on the model's mesh)."""
from absolutetrack_amd.hand import skin_landmarks, skin_mesh  # noqa: F401

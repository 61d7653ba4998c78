"""lib/common/hand_skinning.py of the reference -> the HIP FK kernels (absolutetrack_amd.hand.skin_landmarks, and
skin_mesh: the reference's _skin_points on the model's mesh; render_mesh / overlay: that mesh drawn into crop cameras)."""
from absolutetrack_amd.hand import overlay, render_mesh, skin_landmarks, skin_mesh  # noqa: F401

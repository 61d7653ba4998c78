"""lib/tracker/perspective_crop.py of the reference -> absolutetrack_amd.tracker (project_landmarks / render_hand_pose: the
tracked hand back in the cameras, csrc/render.hip; triangulate_landmarks: the way back, csrc/triangulate.hip)."""
from absolutetrack_amd.tracker import (  # noqa: F401
    gen_crop_cameras_from_pose, landmarks_from_hand_pose, neutral_joint_angles, project_landmarks, rank_hand_visibility_in_cameras,
    render_hand_pose, skin_landmarks_np, triangulate_landmarks)

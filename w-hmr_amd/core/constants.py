"""Constants of the hot path (values of core/constants.py:4-8,16-92 and models/smpl.py:57-58 in the reference)."""
FOCAL_LENGTH = 1000.
IMG_NORM_MEAN = [0.485, 0.456, 0.406]
IMG_NORM_STD = [0.229, 0.224, 0.225]

# Index of each of the 49 named joints inside the 54-joint superset (24 SMPL + 21 picked vertices + 9 regressed);
# order = reference JOINT_NAMES (25 OpenPose + 24 dataset joints), values = its JOINT_MAP.
JOINT_MAP_49 = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7,
                25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53,
                24, 26, 25, 28, 27]
# smplx vertex_ids['smplh'] in VertexJointSelector order (face, feet, finger tips)
EXTRA_VERTEX_IDS = [332, 6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787,
                    2746, 2319, 2445, 2556, 2673, 6191, 5782, 5905, 6016, 6133]
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
H36M_TO_J17 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10, 0, 7, 9]
H36M_TO_J14 = H36M_TO_J17[:14]

# Left / right mirror of the joint sets (augmentation flip; values of core/constants.py:106-118 in the reference, stated per convention):
# out[i] = in[PERM[i]].  SMPL's 24 kinematic joints: pelvis, spine and head chain stay, every left / right pair (hips 1 / 2, knees 4 / 5, ankles
# 7 / 8, feet 10 / 11, collars 13 / 14, shoulders 16 / 17, elbows 18 / 19, wrists 20 / 21, hands 22 / 23) swaps.
SMPL_JOINTS_FLIP_PERM = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]
SMPL_POSE_FLIP_PERM = [3 * j + k for j in SMPL_JOINTS_FLIP_PERM for k in range(3)]           # the 72 axis-angle components, joint by joint
# the 24 dataset joints (right leg 0-2 <-> left leg 5-3, right arm 6-8 <-> left arm 11-9, neck .. head top stay, eyes 19 / 20 and ears 21 / 22 ... swap)
J24_FLIP_PERM = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22]
# the 25 OpenPose joints (arms 2-4 <-> 5-7, legs 9-11 <-> 12-14, eyes, ears, feet 19-21 <-> 22-24)
OPENPOSE25_FLIP_PERM = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21]
J49_FLIP_PERM = OPENPOSE25_FLIP_PERM + [25 + j for j in J24_FLIP_PERM]
SMPL_J49_FLIP_PERM = OPENPOSE25_FLIP_PERM + [25 + j for j in SMPL_JOINTS_FLIP_PERM]

# The 25 bones of the keypoint skeleton the demo draws (--draw_keypoints): the joint pairs of get_spin_skeleton() (datasets/data_utils/kp_utils.py:286
# in the reference) over the 49 joints above -- the OpenPose body, face and feet, and nose -> head top.  tests/golden/skeleton.npz holds the table.
SPIN_SKELETON = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (10, 11), (8, 12), (12, 13), (13, 14), (0, 15), (0, 16),
                 (15, 17), (16, 18), (21, 19), (19, 20), (14, 21), (11, 24), (24, 22), (22, 23), (0, 38)]
# The side of every bone, from the names of get_spin_joint_names() (:212): 'l' / 'r' if one of its two joints is a left / right one ('OP LKnee',
# 'OP RHeel', ...; no bone joins a left joint to a right one), 'c' for the trunk, the neck and the head top.
SPIN_BONE_SIDE = 'crrrlllcrrrlllrlrllllrrrc'
# How the skeleton is drawn is this package's choice (the reference draws it with PARE's draw_skeleton on cv2, neither of them in its tree): the
# person's left warm, the right cold, the centre line yellow, joints white; widths in pixels.
SKELETON_SIDE_RGB = {'l': (1.0, 0.45, 0.2), 'r': (0.2, 0.7, 1.0), 'c': (0.95, 0.9, 0.3)}
SKELETON_JOINT_RGB = (1.0, 1.0, 1.0)
SKELETON_BONE_WIDTH, SKELETON_JOINT_RADIUS = 3.0, 3.0
WIREFRAME_LINE_WIDTH = 1.0

"""Cityscapes constants the hot path consumes (reference datasets/Cityscapes/settings.py:3-30, restated as data)."""
NUM_CLASSES = 19
MEAN = (0.28690, 0.32513, 0.28389)
STD = (0.17614, 0.18099, 0.17772)
IGNORE_CLASS_LABEL = 255
# raw Cityscapes label id -> train id (datasets/Cityscapes/settings.py:9-18)
LABEL_MAPPING_DICT = {
    **{k: IGNORE_CLASS_LABEL for k in (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1)},
    7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15,
    31: 16, 32: 17, 33: 18,
}
# train id -> RGB of the public Cityscapes label table (cityscapesScripts, helpers/labels.py); the ignore label is drawn black
CLASS_RGB_COLOR = {
    0: (128, 64, 128),      # road
    1: (244, 35, 232),      # sidewalk
    2: (70, 70, 70),        # building
    3: (102, 102, 156),     # wall
    4: (190, 153, 153),     # fence
    5: (153, 153, 153),     # pole
    6: (250, 170, 30),      # traffic light
    7: (220, 220, 0),       # traffic sign
    8: (107, 142, 35),      # vegetation
    9: (152, 251, 152),     # terrain
    10: (70, 130, 180),     # sky
    11: (220, 20, 60),      # person
    12: (255, 0, 0),        # rider
    13: (0, 0, 142),        # car
    14: (0, 0, 70),         # truck
    15: (0, 60, 100),       # bus
    16: (0, 80, 100),       # train
    17: (0, 0, 230),        # motorcycle
    18: (119, 11, 32),      # bicycle
    IGNORE_CLASS_LABEL: (0, 0, 0),
}
# train-id names in train-id order (the same public label table)
CLASS_NAMES = ('road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign', 'vegetation', 'terrain', 'sky', 'person',
               'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')

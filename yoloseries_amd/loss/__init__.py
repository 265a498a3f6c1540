from .yolov5_loss import YOLOV5Loss  # noqa: F401
from .yolox_loss import YOLOXLoss  # noqa: F401
from .yolov8_loss import YOLOV8Loss  # noqa: F401
from .yolov7_loss import YOLOV7Loss  # noqa: F401

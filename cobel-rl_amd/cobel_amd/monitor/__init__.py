from .behavior import (EscapeLatencyMonitor, Monitor, QMonitor, ResponseMonitor,  # noqa: F401
                       RewardMonitor, TrajectoryMonitor)
from .network import RepresentationMonitor  # noqa: F401
from .trajectory import TrajectoryRecord  # noqa: F401

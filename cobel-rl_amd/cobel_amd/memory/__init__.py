from .adqn import ADQNMemory  # noqa: F401
from .dqn import DQNMemory  # noqa: F401
from .dyna_q import DynaQMemory  # noqa: F401
from .pma import PMAMemory  # noqa: F401
from .sfma import SFMAMemory  # noqa: F401

from .greedy import EpsilonGreedy, ExclusiveEpsilonGreedy  # noqa: F401
from .policy import Policy  # noqa: F401
from .random import RandomDiscrete  # noqa: F401
from .scalar import Proportional, Sigmoid, Threshold  # noqa: F401
from .softmax import Softmax  # noqa: F401

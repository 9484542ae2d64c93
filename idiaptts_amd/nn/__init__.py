from .modules import (GRU, LSTM, RNN, AllPassWarp, GradientScaling, LinearAct, MeanPooling,  # noqa: F401
                      MLPGLayer, SelectLastPooling, VanillaVAE)
from .wavenet import WaveNet  # noqa: F401

from .modules import (GRU, LSTM, RNN, AllPassWarp, GradientScaling, LinearAct, MeanPooling,  # noqa: F401
                      MLPGLayer, SelectLastPooling, TransformerEncoderLayer, VanillaVAE)
from .wavenet import WaveNet  # noqa: F401

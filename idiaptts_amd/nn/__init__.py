from .modules import GRU, LSTM, RNN, AllPassWarp, GradientScaling, LinearAct  # noqa: F401

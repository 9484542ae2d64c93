"""CategoryDataReader with the reference's interface (data_preparation/CategoryDataReader.py): a reader without
files, `reader[id]` is `{name: id_to_category_fn(id)}`.  It needs no directory and no normalisation; the function's
array -- for classification an int64 class index of shape (1,) or (1, 1) -- travels as it is: the dataset matches no
length to it (no `match_length`), prepare_batch pads it into an int64 [B, 1] (time-major [1, B]) batch, and the
device batch cache keeps anything that is not a [T, D] float32 stream as a host value."""
from idiaptts_amd.src.data_preparation.DataReaderConfig import DataReaderConfig
from idiaptts_amd.src.data_preparation.NpzDataReader import DataReader


class CategoryDataReader(DataReader):

    class Config(DataReader.Config):
        def __init__(self, name, id_to_category_fn):
            super().__init__(name, output_names=DataReaderConfig._str_to_list(name))
            self.id_to_category_fn = id_to_category_fn

        def create_reader(self):
            return CategoryDataReader(self)

    def __init__(self, config):
        super().__init__(config)
        self.id_to_category_fn = config.id_to_category_fn

    def load(self, id_name):
        return self.id_to_category_fn(id_name)

    def preprocess_sample(self, sample):
        return sample

    def __getitem__(self, id_name):
        return {self.name: self.id_to_category_fn(id_name)}

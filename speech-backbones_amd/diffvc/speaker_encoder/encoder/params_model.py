"""Model constants of the speaker encoder (same names and values as DiffVC/speaker_encoder/encoder/params_model.py)."""
model_hidden_size = 256
model_embedding_size = 256
model_num_layers = 3

# GE2E training (not run by this package; kept so that code reading them keeps working)
learning_rate_init = 1e-4
speakers_per_batch = 64
utterances_per_speaker = 10

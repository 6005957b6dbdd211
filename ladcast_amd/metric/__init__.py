from .loss import LpLoss, MSELoss
from .utils import process_tensor_for_loss, remove_channel
